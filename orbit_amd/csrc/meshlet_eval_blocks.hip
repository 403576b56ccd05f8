// meshlet_eval_blocks.hip — the pass-0 evaluation that decides most meshlets per block of 32 (block_pretest.h): the launch
// a single-view orbit_meshlet_cull takes for occlusion pass 0, perspective, canonical arithmetic, from derived streams
// with alpha classes and block bounds.  Everything else keeps meshlet_eval.hip's kernels.
//
// Same wave tile, slabs, pipeline and ticket scheme as meshlet_eval_body, same outputs (tile_masks, tile_counts, zeroed
// chunk sums, status latches).  What differs is a row whose two records are SPARSE (block_record_setup: affine matrix,
// 32-aligned record inside the stream, valid block bound, block small against its distance from the camera): its lanes
// load only the 4-byte cone word and run block_pretest_terms — about 25 vector instructions instead of the literal
// evaluation's 114 and 4 bytes instead of 20.  A lane whose cone verdict is certain and, if kept, whose block is
// certainly inside every plane is decided there; the others ("candidates") go to a wave-private LDS ring as (row, lane)
// codes and are evaluated literally, 64 at a time on full lanes, from gathered sphere + cone reads (eval_geometry_mask:
// the reference's arithmetic, so the result is what the dense row would have given, bit for bit).  Dense rows run
// rows_eval unchanged.
//
// A tile whose eight rows are all sparse has its eight cone words loaded together, a whole tile ahead (issued before the
// tile in front of it runs its rows) and with no sphere load at all; a tile with a dense row keeps the row-by-row
// pipeline, two rows in flight.  Either kind issues the next tile's first loads in the form that tile needs (PipeRegs).
#include "block_pretest.h"
#include "meshlet_common.h"

namespace orbit {

namespace {

constexpr int kBkWaves = 4;
constexpr int kBkWavesPerSimd = 5; // as the kernel this one stands in for (meshlet_eval.hip ORBIT_EV_WPS0)
// candidates are flushed in 64s once 64 are queued — checked after rows 1 and 3, where few registers are live — and at
// the end of the tile, behind the next slab's setup: at most 63 + 4 x 64 are ever queued
constexpr uint32_t kBkRing = 512, kBkFlush = 64;

struct __attribute__((aligned(16))) BlockTileLds {
    BlockRecord r[kTileRecords];
};
struct CandRing {
    uint16_t code[kBkRing]; // row * 64 + lane
};
struct RingState {
    uint32_t head = 0, count = 0; // wave-uniform
    uint32_t total = 0;           // survivors of the tile so far
};

// bit 2 r of the slab's spare word: both records of row r are sparse (blk_setup)
__device__ __forceinline__ bool row_is_sparse(const WaveTileLds &L, int r) {
    const uint32_t w = reinterpret_cast<const uint32_t *>(&L.pad_)[0];
    return (((uint32_t)__builtin_amdgcn_readfirstlane((int)w) >> (2 * r)) & 1u) != 0u;
}

// The block bound of a lane's record (`rec` is held by lanes 4 record .. 4 record + 3, and so is its bound: the four lanes
// of blk_setup's quad), and whether the record starts a block and lies inside the stream.  Unconditional loads: everybody
// else reads the zero page.
struct BoundRegs {
    float4 q; // centre, BlockBound::packed (0, not valid, also where the record is not covered: the zero page)
};
__device__ __forceinline__ BoundRegs blk_load_bound(const MeshletCullParams &p, const BlockBound *blk, const uint4 &rec) {
    const uint32_t y = rec.y, z = rec.z;
    const uint32_t rel = y - p.ms.first;
    BoundRegs b;
    const bool covered = z != 0u && (y & 31u) == 0u && rel < p.ms.count && z <= p.ms.count - rel;
    const float4 *src = covered ? reinterpret_cast<const float4 *>(blk + (y >> 5)) : reinterpret_cast<const float4 *>(p.zero_page);
    b.q = src[0];
    return b;
}

// lane K of the caller's quad's x (quad_perm broadcast, as setup_write_cls)
template <int K>
__device__ __forceinline__ float quad_bcast(float x) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), K * 0x55, 0xF, 0xF, false));
}

// Behind setup_write of the same slab (which ends in a wave barrier): the four lanes that hold record lane >> 2 (`rec`,
// `bb`) derive its BlockRecord — block_pretest.h's quad form, which says who computes what and why the bits are
// block_record_setup's.  plane_nn: block_plane_norm of the planes in use (the kernel's prologue).
__device__ __forceinline__ void blk_setup(const MeshletCullParams &p, WaveTileLds &L, BlockTileLds &B, const PlaneLds &P,
                                          const float *plane_nn, const uint4 &rec, const BoundRegs &bb, int lane) {
    const int rid = lane >> 2, k = lane & 3;
    const RecordLds &R = L.r[rid];
    const float *mf = reinterpret_cast<const float *>(R.mcol);
    const float row[4] = {mf[k], mf[4 + k], mf[8 + k], mf[12 + k]};
    const float4 ca = R.mcol[block_quad_col_a(k)], cb = R.mcol[block_quad_col_b(k)];
    const float a[3] = {ca.x, ca.y, ca.z}, bcol[3] = {cb.x, cb.y, cb.z};
    const BlockBound b = block_bound_unpack(bb.q.x, bb.q.y, bb.q.z, __float_as_uint(bb.q.w));
    const BlockQuadShare s = block_quad_share(row, a, bcol, b.cx, b.cy, b.cz);
    const BlockQuadSums q = {quad_bcast<0>(s.d),  quad_bcast<1>(s.d),  quad_bcast<2>(s.d),  quad_bcast<0>(s.ap),
                             quad_bcast<1>(s.ap), quad_bcast<2>(s.ap), quad_bcast<0>(s.gd), quad_bcast<1>(s.gd),
                             quad_bcast<2>(s.gd), quad_bcast<0>(s.go), quad_bcast<1>(s.go), quad_bcast<3>(s.go)};
    const uint32_t aw = reinterpret_cast<const uint32_t *>(&L.affine_rows)[lane >> 5];
    const bool affine = ((aw >> (8 * ((lane >> 3) & 3))) & 1u) != 0u;
    // (covered: a record that is not reads the zero page, whose bound is not valid)
    const BlockQuadTail t = block_quad_tail(q, affine, R.scale, b, true, ORBIT_BLK_RATIO);
    reinterpret_cast<float *>(&B.r[rid])[k] = block_quad_out(k, a, q, t); // gx, gy, gz, dk
    const uint32_t n = min(p.ci.cull_plane_count, (uint32_t)ORBIT_MAX_CULL_PLANES);
    bool pass = true;
    for (uint32_t i0 = 0; i0 < n; i0 += 4u) { // plane i0 + k
        const bool has = i0 + (uint32_t)k < n;
        const uint32_t i = has ? i0 + (uint32_t)k : 0u;
        const float4 pl4 = P.plane[i];
        const float pl[4] = {pl4.x, pl4.y, pl4.z, pl4.w};
        pass &= block_quad_plane(pl, plane_nn[i], q, t) | !has; // (no branch: a lane without a plane reads plane 0)
    }
    uint64_t in = ballot(pass);
    in &= in >> 1;
    in &= in >> 2; // bit 4 record: every lane of the quad
    const bool none = rec.z == 0u; // no record: no lane of it is ever allowed, it holds no row back
    if (k == 0) {
        const uint32_t flags = none ? kBlkSparse : (t.sparse ? kBlkSparse | (lane_of(in) ? kBlkInside : 0u) : 0u);
        reinterpret_cast<float4 *>(&B.r[rid])[1] = make_float4(t.sigma, t.bk, t.rr, __uint_as_float(flags));
    }
    uint64_t m = ballot(t.sparse || none); // four equal bits per record, eight lanes per row
    m &= m >> 4;                           // bit 8 r: both records of row r
    m &= 0x0101010101010101ull;            // ... moved to bit 2 r, the word row_is_sparse and tile_is_sparse read
    m = (m | m >> 6) & 0x0005000500050005ull;
    m = (m | m >> 12) & 0x0000005500000055ull;
    m = (m | m >> 24) & 0x5555ull;
    if (lane == 0) L.pad_ = m;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The registers the pipeline carries from tile to tile, in one of two forms (wave-uniform, `whole` in the kernel):
// rows: v[0..3] the sphere and v[4] the cone word of row 0 of the tile, v[5..9] the same of row 1 (rows 2.. follow row by
//       row, two in flight, as in meshlet_eval_body);
// whole: v[r] the cone word of row r of an ALL-SPARSE tile — a cone word is one register where a dense row is five, so
//       the eight rows of such a tile fit where two dense rows would, and all eight loads are in flight at once.
struct PipeRegs {
    uint32_t v[10];
};

// every row of the tile is sparse (blk_setup; a tile past the wave's last holds no record and is one, too)
__device__ __forceinline__ bool tile_is_sparse(const WaveTileLds &L) {
    const uint32_t w = reinterpret_cast<const uint32_t *>(&L.pad_)[0];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)w) == 0x5555u;
}

// rows_load<0, R, 1, true, true> into v[0..4], with the sphere read only for a dense row (`sparse` is wave-uniform; the
// load is issued either way, outside the resource for a sparse row, so the wait counts stay exact)
template <int R>
__device__ __forceinline__ void blk_row_load(const MeshletCullParams &p, const WaveTileLds &L, bool sparse, int lane,
                                             uint32_t *v, const StreamRsrc &SR) {
    const uint32_t half = lane >> 5, ml = lane & 31;
    const uint4 rec = L.r[2 * R + half].rec;
    const bool active = ml < rec.z;
    const uint32_t rel = rec.y + ml - SR.first;
    const bool in = active & (rel < SR.count);
    if (active & !in) latch_status(p.status, ORBIT_E_RANGE);
    const uint32_t i = in ? rel : kNoOffset >> 4;
    const uint32_t is = sparse ? kNoOffset >> 4 : i;
    const auto sp = __builtin_amdgcn_raw_buffer_load_b128(SR.sphere, is << 4, 0, ORBIT_EVAL_LOAD_AUX);
    v[4] = __builtin_amdgcn_raw_buffer_load_b32(SR.cone, i << 2, 0, ORBIT_EVAL_LOAD_AUX);
    v[0] = sp[0], v[1] = sp[1], v[2] = sp[2], v[3] = sp[3];
}

// The eight cone words of an all-sparse tile into v[0..7]: eight loads back to back, no sphere load at all.  No range
// check as blk_row_load has it: a record with meshlets is sparse only if blk_load_bound found it covered — inside the
// stream with all its meshlets — so no active lane of such a tile can lie outside (uncovered records make dense rows).
__device__ __forceinline__ void blk_tile_load(const WaveTileLds &L, int lane, uint32_t *v, const StreamRsrc &SR) {
    const uint32_t half = lane >> 5, ml = lane & 31;
#pragma unroll
    for (int r = 0; r < (int)kTileRows; r++) {
        const uint4 rec = L.r[2 * r + half].rec;
        const uint32_t i = ml < rec.z ? rec.y + ml - SR.first : kNoOffset >> 4;
        v[r] = __builtin_amdgcn_raw_buffer_load_b32(SR.cone, i << 2, 0, ORBIT_EVAL_LOAD_AUX);
    }
}

// A dense row from v[0..4]: rows_eval unchanged.
template <int R>
__device__ __forceinline__ uint32_t blk_row_dense(const MeshletCullParams &p, WaveTileLds &L, const PlaneLds &P, int lane,
                                                  const uint32_t *v, uint32_t total) {
    RowRegs<1> t;
    t.a[0] = make_uint4(v[0], v[1], v[2], v[3]);
    t.b[0] = make_uint4(v[4], 0u, 0u, 0u);
    t.prev[0] = 0u;
    return rows_eval<0, 0, R, 1, true>(p, L, P, nullptr, lane, t, total, nullptr);
}

// A sparse row from its cone words: the pre-test decides, the open lanes queue up.
template <int R>
__device__ __forceinline__ void blk_row_eval(WaveTileLds &L, const BlockTileLds &B, CandRing &ring, int lane,
                                             uint32_t cone, RingState &rs) {
    const uint32_t half = lane >> 5;
    const BlockRecord br = B.r[2 * R + half];
    float s0, band;
    block_pretest_terms(br, cone, s0, band);
    const uint64_t culled = ballot(block_cone_culls(br, s0, band));
    const uint64_t kept = ballot(block_cone_keeps(s0, band)) & ballot((br.flags & kBlkInside) != 0u);
    // lanes that hold a meshlet whose material passes (:207), as in rows_eval
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.r[2 * R].amask.x);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)L.r[2 * R + 1].amask.x);
    const uint64_t allow = (uint64_t)hi << 32 | lo;
    const uint64_t draw = allow & kept & ~culled;
    const uint64_t cand = allow & ~culled & ~kept;
    if (lane == 0) L.draw_mask[R] = draw;
    rs.total += (uint32_t)__popcll(draw);
    if (lane_of(cand)) ring.code[(rs.head + rs.count + lane_prefix(cand)) & (kBkRing - 1u)] = (uint16_t)(R * 64 + lane);
    rs.count += (uint32_t)__popcll(cand);
}

// The literal evaluation of the first n <= 64 queued candidates; lane j takes candidate j.  In two steps, so that the
// end-of-tile flush can have its gather in flight while the slab of the tile after the next is set up: blk_flush_load
// reads the codes and issues the gather (n = 0: every lane reads outside the resources), blk_flush_eval evaluates.
struct FlushRegs {
    uint32_t sp[4], c; // sphere and cone word; a lane without a candidate holds zeros
    uint32_t rid, ml;
    bool valid;
};
__device__ __forceinline__ FlushRegs blk_flush_load(const WaveTileLds &L, const CandRing &ring, const StreamRsrc &SR, int lane,
                                                    const RingState &rs, uint32_t n) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    FlushRegs f;
    f.valid = (uint32_t)lane < n;
    const uint32_t code = f.valid ? (uint32_t)ring.code[(rs.head + (uint32_t)lane) & (kBkRing - 1u)] : 0u;
    f.rid = (code >> 5) & 15u, f.ml = code & 31u;
    const uint4 rec = L.r[f.rid].rec;
    const uint32_t rel = rec.y + f.ml - SR.first;
    const uint32_t i = (f.valid && f.ml < rec.z && rel < SR.count) ? rel : kNoOffset >> 4; // (a sparse record lies inside)
    const auto sp = __builtin_amdgcn_raw_buffer_load_b128(SR.sphere, i << 4, 0, 0);
    f.c = __builtin_amdgcn_raw_buffer_load_b32(SR.cone, i << 2, 0, 0);
    f.sp[0] = sp[0], f.sp[1] = sp[1], f.sp[2] = sp[2], f.sp[3] = sp[3];
    return f;
}
__device__ __forceinline__ void blk_flush_eval(const MeshletCullParams &p, WaveTileLds &L, const PlaneLds &P, int lane,
                                               const FlushRegs &f, RingState &rs, uint32_t n) {
    Sphere s;
    // every candidate's record is affine (block_record_setup)
    const uint64_t geo = eval_geometry_mask<0>(p, L, P, f.rid, make_uint4(f.sp[0], f.sp[1], f.sp[2], f.sp[3]),
                                               make_uint4(f.c, 0u, 0u, 0u), s, true);
    const uint64_t vis = geo & ballot(f.valid);
    if (lane_of(vis)) atomicOr(reinterpret_cast<uint32_t *>(L.draw_mask) + f.rid, 1u << f.ml);
    rs.total += (uint32_t)__popcll(vis);
    rs.head = (rs.head + n) & (kBkRing - 1u);
    rs.count -= n;
}
__device__ __forceinline__ void blk_flush(const MeshletCullParams &p, WaveTileLds &L, const PlaneLds &P, const CandRing &ring,
                                          const StreamRsrc &SR, int lane, RingState &rs, uint32_t n) {
    const FlushRegs f = blk_flush_load(L, ring, SR, lane, rs, n);
    blk_flush_eval(p, L, P, lane, f, rs, n);
}

__global__ __launch_bounds__(kBkWaves * 64, kBkWavesPerSimd) void meshlet_eval_blocks_kernel(const MeshletCullParams p,
                                                                                            const BlockBound *blk) {
    __shared__ WaveTileLds lds[kBkWaves][3];
    __shared__ BlockTileLds blds[kBkWaves][2]; // of tile i in [i & 1]: written when tile i - 2 is through its rows
    __shared__ PlaneLds planes;
    __shared__ CandRing rings[kBkWaves];
    __shared__ float plane_nn[ORBIT_MAX_CULL_PLANES]; // block_plane_norm of the planes in use: constant for the launch
    __shared__ uint32_t cls_sel[8]; // [2 c + k] = all ones if alpha class c has predicate bit k (alpha_bits)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the ramp, the tile assignment (static share + tickets) and the priorities: meshlet_eval_body, which explains them
    const uint32_t nrec_raw = *reinterpret_cast<const uint32_t *>(p.dispatch_buffer);
    // (wave-uniform, and told so: the ticket pool and its counter's address then live in scalar registers)
    const uint32_t stride = gridDim.x * kBkWaves, wave_g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kBkWaves + wave));
    const uint32_t cap_tiles = (p.dispatch_capacity + kTileRecords - 1) / kTileRecords;
    uint4 r0 = setup_load_rec(p, wave_g, wave_g < cap_tiles, p.dispatch_capacity, lane);
    uint4 r1 = setup_load_rec(p, wave_g + stride, wave_g + stride < cap_tiles, p.dispatch_capacity, lane);
    uint4 rec2 = setup_load_rec(p, wave_g + 2u * stride, wave_g + 2u * stride < cap_tiles, p.dispatch_capacity, lane);
    planes_to_lds(p, planes);
    if (threadIdx.x < min(p.ci.cull_plane_count, (uint32_t)ORBIT_MAX_CULL_PLANES)) {
        const float *pl = p.ci.cull_planes[threadIdx.x];
        plane_nn[threadIdx.x] = block_plane_norm(pl[0], pl[1], pl[2]);
    }
    clear_chunk_sums(p, kBkWaves * 64);
    if (threadIdx.x < 6) cls_sel[threadIdx.x] = ((alpha_bits(p.ci, threadIdx.x >> 1) >> (threadIdx.x & 1u)) & 1u) ? ~0u : 0u;
    __syncthreads();
    const uint32_t nrec = min(nrec_raw, p.dispatch_capacity);
    const uint32_t ntiles = (nrec + kTileRecords - 1) / kTileRecords;
    const uint32_t full_rounds = ntiles / stride;
    const uint32_t dyn_rounds = min(max(full_rounds / 4u, 1u), 3u);
    const uint32_t n_static = ntiles <= stride ? 0xFFFFFFFFu : max(full_rounds >= dyn_rounds ? full_rounds - dyn_rounds : 0u, 3u);
    const uint32_t npools = min((uint32_t)kTicketPools, stride);
    const uint32_t pool = wave_g % npools;
    uint32_t *ticket_ctr = p.tickets + pool * kTicketStride;
    uint32_t claims = 0;
    auto claim = [&]() -> uint32_t {
        uint32_t raw = claims;
        if (claims >= n_static) {
            raw = 0;
            if (lane == 0) raw = atomicAdd(ticket_ctr, 1u);
        }
        claims++;
        return raw;
    };
    auto ticket_tile = [&](uint32_t raw, uint32_t k) -> uint32_t {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)raw);
        if (k < n_static) return t * stride + wave_g;
        return t >= 0x08000000u ? 0xFFFFFFFFu : n_static * stride + t * npools + pool;
    };
    StreamRsrc SR = {};
    SR.first = p.ms.first;
    SR.count = p.ms.count;
    SR.sphere = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4 *>(p.ms.sphere + p.ms.first), 0, p.ms.count * 16u, kBufFlags);
    SR.cone = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(p.ms.cone + p.ms.first), 0, p.ms.count * 4u, kBufFlags);
    uint32_t w0, w1, w2, tk_raw;
    {
        const uint32_t t0 = claim(), t1 = claim(), t2 = claim();
        tk_raw = claim();
        w0 = ticket_tile(t0, 0u);
        w1 = ticket_tile(t1, 1u);
        w2 = ticket_tile(t2, 2u);
    }
    PipeRegs q;  // tile w0's first loads, in the form `whole` names
    bool whole;  // wave-uniform
    uint32_t *const qa = q.v, *const qb = q.v + 5;
    {
        const uint4 none = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t rl = (uint32_t)lane >> 2;
        if (!(w0 < ntiles && w0 * kTileRecords + rl < nrec)) r0 = none;
        if (!(w1 < ntiles && w1 * kTileRecords + rl < nrec)) r1 = none;
        if (!(w2 < ntiles && w2 * kTileRecords + rl < nrec)) rec2 = none;
        if ((lane & 3) == 0) lds[wave][0].r[lane >> 2].rec = r0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float4 m0 = setup_load_mat(p, r0, lane);
        const float4 m1 = setup_load_mat(p, r1, lane);
        const uint32_t c0 = setup_load_cls(p, r0, lane), c1 = setup_load_cls(p, r1, lane);
        const BoundRegs b0 = blk_load_bound(p, blk, r0), b1 = blk_load_bound(p, blk, r1);
        setup_write_cls(lds[wave][0], cls_sel, r0, c0, lane);
        setup_write_cls(lds[wave][1], cls_sel, r1, c1, lane);
        setup_write(p, lds[wave][0], r0, m0, lane);
        blk_setup(p, lds[wave][0], blds[wave][0], planes, plane_nn, r0, b0, lane);
        // tile 0's first loads go out once its slab says which of its rows are sparse, behind the second slab's loads
        // and ahead of its setup: no sphere is read for a row that never looks at it
        whole = tile_is_sparse(lds[wave][0]);
        if (whole) {
            blk_tile_load(lds[wave][0], lane, q.v, SR);
            q.v[8] = q.v[9] = 0u;
        } else {
            blk_row_load<0>(p, lds[wave][0], row_is_sparse(lds[wave][0], 0), lane, qa, SR);
            blk_row_load<1>(p, lds[wave][0], row_is_sparse(lds[wave][0], 1), lane, qb, SR);
        }
        setup_write(p, lds[wave][1], r1, m1, lane);
        blk_setup(p, lds[wave][1], blds[wave][1], planes, plane_nn, r1, b1, lane);
    }
    uint32_t it = 0;
    const uint32_t prio_rank = blockIdx.x / max(gridDim.x / (uint32_t)kBkWavesPerSimd, 1u);
    while (w0 < ntiles) {
        switch ((it + prio_rank) & 3u) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
        }
        const uint32_t w3 = ticket_tile(tk_raw, claims - 1u);
        tk_raw = claim();
        WaveTileLds &L = lds[wave][it % 3];
        WaveTileLds &Ln = lds[wave][(it + 1) % 3];
        const BlockTileLds &B = blds[wave][it & 1u];
        CandRing &ring = rings[wave];
        RingState rs;
        // the next tile's slab is complete (blk_setup runs two tiles ahead): its loads go out in the form it needs
        const bool nxt_whole = tile_is_sparse(Ln);
        float4 mat2;
        uint32_t cls2;
        BoundRegs bnd2;
        uint4 rec3;
        // The setup loads of the tile after the next: they depend only on rec2, which landed a tile ago.
#define BK_SETUP_LOADS()                                                                                               \
    mat2 = setup_load_mat(p, rec2, lane);                                                                              \
    cls2 = setup_load_cls(p, rec2, lane);                                                                              \
    bnd2 = blk_load_bound(p, blk, rec2);                                                                               \
    rec3 = setup_load_rec(p, w3, w3 < ntiles, nrec, lane);
#define BK_FLUSH() \
    while (rs.count >= kBkFlush) blk_flush(p, L, planes, ring, SR, lane, rs, kBkFlush);
        if (whole) {
            // An all-sparse tile: its eight cone words are in q.  The setup loads go out FIRST: a wait the compiler attaches
            // to their address arithmetic then covers nothing fresh, where behind the next tile's loads the same wait
            // makes those land (vector loads return in order) — a full memory round trip at the top of every tile.  They
            // are consumed behind the rows (setup_write_cls, setup_write, blk_setup below).  Then the next tile's loads,
            // then the eight rows from registers with no load between them.  Each arm of `if (nxt_whole)` has its own
            // straight-line copy of the rows: the compiler's vmcnt counts are per path, and behind a merge of an arm with
            // eight loads in flight and one with four the first row would wait for the smaller count — half of the loads
            // just issued.  In the steady arm (an all-sparse tile behind an all-sparse tile) nothing waits for them.
#define BK_SPARSE_ROWS()                                                                                               \
    blk_row_eval<0>(L, B, ring, lane, q.v[0], rs);                                                                     \
    blk_row_eval<1>(L, B, ring, lane, q.v[1], rs);                                                                     \
    BK_FLUSH()                                                                                                         \
    blk_row_eval<2>(L, B, ring, lane, q.v[2], rs);                                                                     \
    blk_row_eval<3>(L, B, ring, lane, q.v[3], rs);                                                                     \
    BK_FLUSH()                                                                                                         \
    blk_row_eval<4>(L, B, ring, lane, q.v[4], rs);                                                                     \
    blk_row_eval<5>(L, B, ring, lane, q.v[5], rs);                                                                     \
    blk_row_eval<6>(L, B, ring, lane, q.v[6], rs);                                                                     \
    blk_row_eval<7>(L, B, ring, lane, q.v[7], rs);
            BK_SETUP_LOADS()
            PipeRegs tn;
            if (nxt_whole) {
                blk_tile_load(Ln, lane, tn.v, SR);
                tn.v[8] = tn.v[9] = 0u;
                BK_SPARSE_ROWS()
            } else {
                blk_row_load<0>(p, Ln, row_is_sparse(Ln, 0), lane, tn.v, SR);
                blk_row_load<1>(p, Ln, row_is_sparse(Ln, 1), lane, tn.v + 5, SR);
                BK_SPARSE_ROWS()
            }
#undef BK_SPARSE_ROWS
            q = tn;
        } else {
            // A tile with a dense row: row by row, two in flight, as before.  The next tile's loads go out where the
            // row registers fall free: rows 0 and 1 behind rows 6 and 7, a whole tile of cone words behind row 7.
#define BK_ROW(R, Q)                                                                                                   \
    if (row_is_sparse(L, R)) blk_row_eval<R>(L, B, ring, lane, (Q)[4], rs);                                            \
    else rs.total = blk_row_dense<R>(p, L, planes, lane, Q, rs.total);
            BK_ROW(0, qa)
            blk_row_load<2>(p, L, row_is_sparse(L, 2), lane, qa, SR);
            BK_ROW(1, qb)
            blk_row_load<3>(p, L, row_is_sparse(L, 3), lane, qb, SR);
            BK_FLUSH()
            BK_ROW(2, qa)
            blk_row_load<4>(p, L, row_is_sparse(L, 4), lane, qa, SR);
            BK_ROW(3, qb)
            blk_row_load<5>(p, L, row_is_sparse(L, 5), lane, qb, SR);
            BK_FLUSH()
            BK_SETUP_LOADS() // (where the row registers allow: behind this tile's own row loads, never behind the next tile's)
            BK_ROW(4, qa)
            blk_row_load<6>(p, L, row_is_sparse(L, 6), lane, qa, SR);
            BK_ROW(5, qb)
            blk_row_load<7>(p, L, row_is_sparse(L, 7), lane, qb, SR);
            BK_ROW(6, qa)
            if (!nxt_whole) blk_row_load<0>(p, Ln, row_is_sparse(Ln, 0), lane, qa, SR);
            BK_ROW(7, qb)
            if (nxt_whole) {
                blk_tile_load(Ln, lane, q.v, SR);
                q.v[8] = q.v[9] = 0u;
            } else {
                blk_row_load<1>(p, Ln, row_is_sparse(Ln, 1), lane, qb, SR);
            }
#undef BK_ROW
        }
#undef BK_FLUSH
#undef BK_SETUP_LOADS
        whole = nxt_whole;
        // The candidates still queued (from bench.py's camera about nine a tile, never 64): the gather of the first 64 goes
        // out HERE and is evaluated behind the slab's setup, which neither reads nor writes what the evaluation touches
        // (this tile's slab L and its masks) — so the gather's round trip, which nothing else hid, runs under some 150
        // instructions of setup instead of in front of an s_waitcnt.  Issued for no candidate too: straight-line code.
        const uint32_t n_end = min(rs.count, kBkFlush);
        const FlushRegs fl_end = blk_flush_load(L, ring, SR, lane, rs, n_end);
        setup_write_cls(lds[wave][(it + 2) % 3], cls_sel, rec2, cls2, lane);
        setup_write(p, lds[wave][(it + 2) % 3], rec2, mat2, lane);
        blk_setup(p, lds[wave][(it + 2) % 3], blds[wave][it & 1u], planes, plane_nn, rec2, bnd2, lane); // (this tile's rows are through)
        if (n_end > 0u) blk_flush_eval(p, L, planes, lane, fl_end, rs, n_end);
        while (rs.count > 0u) blk_flush(p, L, planes, ring, SR, lane, rs, min(rs.count, kBkFlush));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the mask writes of this tile
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < 2 * (int)kTileRows)
            p.tile_masks[(size_t)w0 * (2 * kTileRows) + lane] = reinterpret_cast<const uint32_t *>(L.draw_mask)[lane];
        if (lane == 0) p.tile_counts[w0] = rs.total;
        w0 = w1;
        w1 = w2;
        w2 = w3;
        rec2 = rec3;
        it++;
    }
}

} // namespace

// `grid`: meshlet_eval.hip's for this pass and source (launch_meshlet_eval sizes it)
hipError_t launch_meshlet_eval_blocks(const MeshletCullParams &p, const BlockBound *blk, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL(meshlet_eval_blocks_kernel, grid, dim3(kBkWaves * 64), 0, s, p, blk);
    return hipGetLastError();
}

} // namespace orbit
