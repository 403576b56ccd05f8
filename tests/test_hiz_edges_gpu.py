"""The pass-2 HiZ test (occlusion_test -> project_sphere -> hiz_sample -> footprint_min, orbit_device.h) at its edges, on
every kernel path and in both forms of the pyramid: the hostile cases of tests/hiz_edges.py — degenerate and non-finite
spheres against pyramids of extreme aspect holding NaN, +-inf, negative and arbitrary texels; what each case exercises is
counted by tests/test_hiz_edges_cpu.py — bit for bit against the oracle.

Every packed pyramid here lives INSIDE a larger device buffer whose texels before and after it are -inf, and every
per-mip image has -inf padding, a -inf row above and one below: a read that strays off the pyramid samples -inf, which
turns a culled row visible, and the guards are checked to be untouched afterwards."""
import numpy as np
import pytest

import cull_stats_ref as stats_ref
import hiz_edges as hz
from orbit_amd import layouts as L
from test_gpu_parity import GpuScene, _expected_visible_records, assert_same, dev, host, run_oracle, torch_mod  # noqa: F401
from test_hiz_edges_cpu import load_case, load_contracted, vectors  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = ["meshlet_buffer", "meshlet_stream", "meshlet_stream_classes", "one_launch"]
CAPS = dict(max_entities=8192, max_dispatches=60_000, max_draws=400_000)
GUARD = 4096  # texels of -inf on either side of a packed pyramid
LEVEL_T = np.dtype([("texels", "<u8"), ("row_pitch", "<u4"), ("_pad", "<u4")])  # OrbitDepthPyramidLevel


def make_engine(path, **caps):
    from orbit_amd.engine import Engine
    from stream_engine import StreamEngine

    kw = dict(CAPS, **caps)
    if path == "one_launch":  # entity + meshlet stage as ONE launch (cull_fused.hip)
        from fused_engine import FusedEngine

        return FusedEngine(0, **kw)
    return Engine(0, **kw) if path == "meshlet_buffer" else StreamEngine(0, classes=path == "meshlet_stream_classes", **kw)


class _Engines:
    """The engine of one path in either arithmetic profile, made when first asked for."""

    def __init__(self, path):
        self.path, self.made = path, {}

    def __getitem__(self, profile):
        if profile not in self.made:
            self.made[profile] = make_engine(self.path, arith_profile=profile)
        return self.made[profile]


@pytest.fixture(scope="module", params=PATHS)
def engines(torch_mod, request):
    e = _Engines(request.param)
    yield e
    for eng in e.made.values():
        eng.close()


@pytest.fixture(scope="module")
def engine(engines):
    return engines[0]


@pytest.fixture(scope="module")
def engine_contracted(engines):
    return engines[1]


@pytest.fixture(scope="module")
def plain(torch_mod):
    e = make_engine("meshlet_buffer")
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ guarded pyramids
class Packed:
    """The packed chain between two guards of -inf."""

    def __init__(self, torch, pyr, psize):
        self.torch, self.n, self.psize = torch, len(pyr), psize
        self.buf = torch.full((GUARD + self.n + GUARD,), float("-inf"), dtype=torch.float32, device="cuda")
        self.want = torch.from_numpy(np.ascontiguousarray(pyr).view(np.int32).copy()).cuda()
        self.buf[GUARD:GUARD + self.n].view(torch.int32).copy_(self.want)

    def kw(self):
        return dict(depth_pyramid=self.buf[GUARD:GUARD + self.n], depth_pyramid_size=self.psize)

    def check(self):
        ninf = float("-inf")
        assert bool((self.buf[:GUARD] == ninf).all()) and bool((self.buf[GUARD + self.n:] == ninf).all()), "a guard was written"
        assert self.torch.equal(self.buf[GUARD:GUARD + self.n].view(self.torch.int32), self.want), "the pyramid was written"


class Levels:
    """One image per mip level with its own padded row pitch (OrbitDepthPyramidLevel), the padding, a row above and a
    row below each image -inf; filled from the packed chain `pyr`, or left at -7 for orbit_depth_reduce_multi to write.
    The device table has one entry more than the pyramid has levels: a guard, an image of -inf."""

    def __init__(self, torch, desc, psize, pyr=None):
        self.torch, self.desc, self.psize, self.images = torch, desc, psize, []
        table = np.zeros(desc.mip_levels + 1, LEVEL_T)
        self.guard = torch.full((3, 8), float("-inf"), dtype=torch.float32, device="cuda")
        table[desc.mip_levels] = (self.guard[1].data_ptr(), 8, 0)
        for k in range(desc.mip_levels):
            w, h, off = desc.mip_width[k], desc.mip_height[k], desc.mip_offset[k]
            pitch = w + (7 if k % 2 else 32)
            t = torch.full((h + 2, pitch), float("-inf"), dtype=torch.float32, device="cuda")
            if pyr is None:
                t[1:h + 1, :w] = -7.0
            else:
                lvl = np.ascontiguousarray(pyr[off:off + w * h]).view(np.int32).reshape(h, w).copy()
                t.view(torch.int32)[1:h + 1, :w].copy_(torch.from_numpy(lvl).cuda())
            self.images.append((t, pitch, w, h, off))
            table[k] = (t[1].data_ptr(), pitch, 0)
        self.table = dev(torch, table)

    def kw(self):
        return dict(depth_pyramid_size=self.psize, depth_pyramid_levels=self.table)

    def reduce_item(self, depth, W, H, depth_row_pitch):
        return dict(depth=depth, width=W, height=H, depth_row_pitch=depth_row_pitch,
                    levels=[(t[1], pitch) for t, pitch, _, _, _ in self.images])

    def check(self, pyr):
        """Level contents == the packed chain `pyr`; the padding and the guard rows untouched."""
        ninf = float("-inf")
        for k, (t, pitch, w, h, off) in enumerate(self.images):
            got = t.cpu().numpy()
            assert np.array_equal(got[1:h + 1, :w].view(np.uint32), pyr[off:off + w * h].reshape(h, w).view(np.uint32)), k
            assert np.all(got[1:h + 1, w:] == ninf) and np.all(got[0] == ninf) and np.all(got[h + 1] == ninf), k


# ---------------------------------------------------------------------------------------------------- shared state
_state = {}


def gpu_case(torch, oracle, name):
    """The case, its scene on the device and its two pyramid forms: built once, read-only afterwards."""
    if name not in _state:
        c = hz.make_case(name, oracle)
        _state[name] = dict(c, gs=GpuScene(torch, c["scene"]), packed=Packed(torch, c["pyr"], c["psize"]),
                            levels=Levels(torch, c["desc"], c["psize"], c["pyr"]))
    return _state[name]


VARIANTS = ["zero_words", "random_words_materials", "entity_only", "frustum", "tilted_planes", "two_planes"]


def variant(c, which):
    """-> (cull info, entity words, meshlet words or None, material_count)."""
    s, cam, ortho = c["scene"], c["cam"], c["ortho"]
    none = np.zeros((0, 4), np.float32)
    if which == "zero_words":
        return (c["ci"],) + hz.words(s, "zero") + (0,)
    if which == "random_words_materials":
        return (hz.cull_info(cam, ortho, none, noskip_alphamode=L.ALPHA_MASKED),) + hz.words(s, "random", 1) + (len(s.materials),)
    if which == "entity_only":  # no meshlet visibility buffer: the entity stage alone tests occlusion
        return hz.cull_info(cam, ortho, none, meshlet_visibility=False), hz.words(s, "random", 2)[0], None, 0
    planes = np.asarray(cam.planes, np.float32).copy()
    if which == "tilted_planes":  # no longer the symmetric frustum: the literal plane loop
        planes[0, 1] = 1e-3
    if which == "two_planes":
        planes = planes[:2]
    return (hz.cull_info(cam, ortho, planes),) + hz.words(s, "random", 3) + (len(s.materials),)


_refs = {}


def reference(oracle, c, which, profile=0):
    key = (c["name"], which, profile)
    if key not in _refs:
        ci, evis, mvis, _ = variant(c, which)
        with oracle.arith_profile(profile):
            _refs[key] = run_oracle(oracle, c["scene"], ci, evis, mvis, c["pyr"], c["psize"])
        assert _refs[key][4] == 0 and _refs[key][5] == 0
    return _refs[key]


def cull(torch, eng, c, which, pyramid_kw):
    """entity_cull + meshlet_cull of a variant -> what assert_same takes."""
    ci, evis, mvis, material_count = variant(c, which)
    s, gs = c["scene"], c["gs"]
    disp_cap, draw_cap = s.max_dispatches() + 8, s.lod0_meshlets + 8
    disp = torch.full((L.DISPATCH_HEADER + 16 * disp_cap + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    draw = torch.full((L.DRAW_HEADER + 28 * draw_cap + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    evis_d = dev(torch, evis)
    mvis_d = None if mvis is None else dev(torch, mvis)
    eng.entity_cull(ci, gs.draws, gs.mesh_infos, disp, gs.entities, s.entity_draw_count, disp_cap, visibility_buffer=evis_d,
                    **pyramid_kw)
    eng.meshlet_cull(ci, disp, gs.meshlets, draw, gs.entities, gs.materials, disp_cap, draw_cap,
                     meshlet_visibility_buffer=mvis_d, material_count=material_count, **pyramid_kw)
    torch.cuda.synchronize()
    eng.status()
    assert bool((disp[L.DISPATCH_HEADER + 16 * disp_cap:] == 0xAB).all()), "write past the dispatch capacity"
    assert bool((draw[L.DRAW_HEADER + 28 * draw_cap:] == 0xCD).all()), "write past the draw capacity"
    return host(disp), host(draw), host(evis_d, np.uint32), None if mvis_d is None else host(mvis_d, np.uint32)


# ------------------------------------------------------------------------------ 1. paths, projections, shapes, variants
@pytest.mark.parametrize("name", list(hz.CASES))
def test_hostile_case_on_every_path(torch_mod, engine, oracle, name):
    """Meshlet buffer, derived streams (with and without alpha classes) and the one-launch cull x perspective and
    orthographic x the pyramids 256x128, 256x16, 16x256, 2x128, 1x1, 4096x32 (13 mips) and 1024x1024 (and the *_floor
    cases, whose collapsed upper levels hold depths that cull): all-zero and random
    visibility words, the alpha table given and not, entity-only occlusion, and cull-plane sets with the symmetric
    frustum's and the affine rows' short cuts on while pass 2 runs."""
    c = gpu_case(torch_mod, oracle, name)
    for which in VARIANTS:
        recs, cmds = assert_same(cull(torch_mod, engine, c, which, c["packed"].kw()), reference(oracle, c, which))
        assert len(recs) > 0 and len(cmds) > 0, which
    c["packed"].check()


# ----------------------------------------------------------------------------------- 2. the remaining entry points
def _task_records_and_list(torch, eng, oracle, c, pyramid_kw, profile=0):
    """orbit_meshlet_task_cull and orbit_meshlet_cull_visible_records on the oracle's dispatch records of a case."""
    which = "random_words_materials"
    ci, evis, mvis, _ = variant(c, which)
    s, gs = c["scene"], c["gs"]
    ref = reference(oracle, c, which, profile)
    cap_d = s.max_dispatches() + 8
    disp = dev(torch, ref[0])
    mvis_d = dev(torch, mvis)
    task = torch.full((44 * cap_d + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.meshlet_task_cull(ci, disp, gs.meshlets, task, gs.entities, gs.materials, cap_d, meshlet_visibility_buffer=mvis_d,
                          **pyramid_kw)
    torch.cuda.synchronize()
    eng.status()
    with oracle.arith_profile(profile):
        orecs, omv = oracle.meshlet_task_cull(ci, ref[0], s.meshlets, s.entities, s.materials, mvis, c["pyr"], c["psize"])
    n = len(orecs)
    assert n > 0 and int(orecs["task_mesh_count"].sum()) > 0
    assert np.array_equal(host(task)[:44 * n], orecs.view(np.uint8).reshape(-1)), "task records differ"
    assert bool((host(task)[44 * n:] == 0xEE).all())
    assert np.array_equal(host(mvis_d, np.uint32), omv), "meshlet visibility words differ (task path)"
    # the record-granular visible list
    mvis_d = dev(torch, mvis)
    vis = torch.full((L.VISIBLE_HEADER + 12 * cap_d + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    eng.meshlet_cull_visible_records(ci, disp, gs.meshlets, vis, gs.entities, gs.materials, cap_d, cap_d,
                                     meshlet_visibility_buffer=mvis_d, **pyramid_kw)
    torch.cuda.synchronize()
    eng.status()
    _, drecs = L.dispatch_buffer_records(ref[0])
    on, ocmds = L.draw_buffer_commands(ref[1])
    want = _expected_visible_records(drecs, ocmds)
    hv = host(vis)
    assert tuple(int(v) for v in hv[:8].view(np.uint32)) == (len(want), on) and on > 0
    assert np.array_equal(hv[8:8 + 12 * len(want)].view(np.uint32), want.view(np.uint32))
    assert bool((hv[8 + 12 * len(want):] == 0xCD).all())
    assert np.array_equal(host(mvis_d, np.uint32), ref[3]), "meshlet visibility words differ (record list)"


def _stats(torch, eng, c, pyramid_kw):
    """orbit_cull_stats against the numpy classifier; the HiZ test must have rejected rows in both stages."""
    from orbit_amd.engine import cull_stats_dict

    which = "random_words_materials"
    ci, evis, mvis, material_count = variant(c, which)
    s, gs = c["scene"], c["gs"]
    want = stats_ref.public(stats_ref.classify(ci, s.entity_draws, s.entity_draw_count, s.entity_draw_count, s.mesh_infos,
                                               s.entities, s.meshlets, s.materials, evis, mvis, c["pyr"], c["psize"]))
    cap_d, cap_c = s.max_dispatches() + 8, s.lod0_meshlets + 8
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device="cuda")
    stats = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
    eng.cull_stats(stats, ci, gs.draws, gs.mesh_infos, disp, gs.entities, s.entity_draw_count, cap_d, gs.meshlets, draw,
                   gs.materials, cap_c, visibility_buffer=dev(torch, evis), meshlet_visibility_buffer=dev(torch, mvis),
                   material_count=material_count, **pyramid_kw)
    torch.cuda.synchronize()
    eng.status()
    got = cull_stats_dict(stats)
    assert got == want
    stats_ref.check_invariants(got)
    assert got["entity_occlusion_culled"] > 0 and got["meshlet_occlusion_culled"] > 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("form", ["packed", "levels"])
@pytest.mark.parametrize("name", list(hz.CASES))
def test_task_cull_visible_records_and_stats(torch_mod, plain, oracle, name, form):
    """orbit_meshlet_task_cull, orbit_meshlet_cull_visible_records and orbit_cull_stats (against tests/cull_stats_ref.py)
    on the hostile cases, from the guarded packed chain and from one image per level."""
    c = gpu_case(torch_mod, oracle, name)
    _task_records_and_list(torch_mod, plain, oracle, c, c[form].kw())
    _stats(torch_mod, plain, c, c[form].kw())
    c["packed"].check()
    c["levels"].check(c["pyr"])


@pytest.mark.parametrize("name", list(hz.CASES))
def test_contracted_profile_on_every_path(torch_mod, engine_contracted, oracle, name):
    """arith_profile = 1 (the *_contracted twins of the cull kernels) against oracle.arith_profile(1), from the packed chain
    and from a level table; the task cull and the record list with it."""
    c = gpu_case(torch_mod, oracle, name)
    for form, which in (("packed", "random_words_materials"), ("levels", "frustum"), ("levels", "zero_words")):
        assert_same(cull(torch_mod, engine_contracted, c, which, c[form].kw()), reference(oracle, c, which, profile=1))
    _task_records_and_list(torch_mod, engine_contracted, oracle, c, c["levels"].kw(), profile=1)
    c["packed"].check()
    c["levels"].check(c["pyr"])


@pytest.mark.parametrize("profile", [0, 1], ids=["canonical", "contracted"])
@pytest.mark.parametrize("name", list(hz.VECTOR_CASES))
def test_product_equals_the_reference_binaries_on_the_hostile_cases(torch_mod, engines, vectors, name, profile):
    """tests/golden/spirv_cull_hiz_edges.npz: the reference's own binaries' records, commands, visibility words and task
    records, on every path and in both profiles."""
    torch = torch_mod
    eng = engines[profile]
    c = load_contracted(vectors, name) if profile else load_case(vectors, name)
    n_draws = int(np.frombuffer(c["draws"][:4].tobytes(), np.uint32)[0])
    cap_d, cap_c = c["caps"]
    g = {k: dev(torch, c[k]) for k in ("draws", "mesh_infos", "entities", "meshlets", "materials")}
    evis, mvis = dev(torch, c["evis"]), dev(torch, c["mvis"])
    pyr = Packed(torch, c["pyr"], c["ps"])
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * cap_d, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(L.DRAW_HEADER + 28 * cap_c, dtype=torch.uint8, device="cuda")
    eng.entity_cull(c["ci"], g["draws"], g["mesh_infos"], disp, g["entities"], n_draws, cap_d, visibility_buffer=evis, **pyr.kw())
    eng.meshlet_cull(c["ci"], disp, g["meshlets"], draw, g["entities"], g["materials"], cap_d, cap_c,
                     meshlet_visibility_buffer=mvis, material_count=len(c["materials"]), **pyr.kw())
    torch.cuda.synchronize()
    eng.status()
    nrec, ndraw = int(c["spv_dispatch"][:4].view(np.uint32)[0]), int(c["spv_draw"][:4].view(np.uint32)[0])
    assert np.array_equal(host(disp)[:L.DISPATCH_HEADER + 16 * nrec], c["spv_dispatch"]), "dispatch records differ"
    assert np.array_equal(host(draw)[:L.DRAW_HEADER + 28 * ndraw], c["spv_draw"]), "draw commands differ"
    assert np.array_equal(host(evis, np.uint32), c["spv_evis"]) and np.array_equal(host(mvis, np.uint32), c["spv_mvis"])
    # the mesh-shading path on the binary's records, from the same visibility words
    mvis_t = dev(torch, c["mvis"])
    disp_t = torch.zeros_like(disp)
    disp_t[:len(c["spv_dispatch"])] = dev(torch, c["spv_dispatch"])
    task = torch.full((44 * cap_d + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    eng.meshlet_task_cull(c["ci"], disp_t, g["meshlets"], task, g["entities"], g["materials"], cap_d,
                          meshlet_visibility_buffer=mvis_t, **pyr.kw())
    torch.cuda.synchronize()
    eng.status()
    n = len(c["spv_task_records"])
    assert np.array_equal(host(task)[:44 * n], c["spv_task_records"].view(np.uint8).reshape(-1)), "task records differ"
    assert np.array_equal(host(mvis_t, np.uint32), c["spv_task_mvis"])
    pyr.check()


# ------------------------------------------------------------------------------------ 4. the per-mip form everywhere
def reduced_levels(torch, eng, c, reduce=True):
    """A pitched depth buffer (NaN padding) reduced by orbit_depth_reduce_multi into fresh per-level images."""
    W, H = c["screen"]
    dpitch = W + 13
    dbuf = torch.full((H, dpitch), float("nan"), dtype=torch.float32, device="cuda")
    dbuf.view(torch.int32)[:, :W] = torch.from_numpy(c["depth"].view(np.int32).copy()).cuda()
    lv = Levels(torch, c["desc"], c["psize"])
    item = lv.reduce_item(dbuf, W, H, dpitch)
    if reduce:
        eng.depth_reduce_multi([item])
    return lv, item, dbuf


@pytest.mark.parametrize("name", list(hz.CASES))
def test_per_mip_images_on_every_path(torch_mod, engine, oracle, name):
    """The pyramid as an image with a view per mip: orbit_depth_reduce_multi writes one padded image per level from a
    pitched hostile depth buffer, then the launch chain, both stream paths and the one-launch cull sample them through
    the device-side level table.  Level contents == the oracle's packed chain, the padding is untouched, the cull
    outputs == the oracle's (which the packed runs of test_hostile_case_on_every_path equal too)."""
    torch = torch_mod
    c = gpu_case(torch, oracle, name)
    lv, _, _ = reduced_levels(torch, engine, c)
    for which in ("zero_words", "random_words_materials", "frustum"):
        assert_same(cull(torch, engine, c, which, lv.kw()), reference(oracle, c, which))
    lv.check(c["pyr"])


def _view(torch, c, which, pyramid_kw):
    ci, evis, mvis, material_count = variant(c, which)
    s, gs = c["scene"], c["gs"]
    disp_cap, draw_cap = s.max_dispatches() + 8, s.lod0_meshlets + 8
    disp = torch.zeros(L.DISPATCH_HEADER + 16 * disp_cap, dtype=torch.uint8, device="cuda")
    draw = torch.zeros(L.DRAW_HEADER + 28 * draw_cap, dtype=torch.uint8, device="cuda")
    e_d, m_d = dev(torch, evis), dev(torch, mvis)
    view = dict(cull_info=ci, entity_draw_buffer=gs.draws, mesh_info_buffer=gs.mesh_infos, meshlet_dispatch_buffer=disp,
                entity_buffer=gs.entities, entity_draw_count=s.entity_draw_count, dispatch_capacity=disp_cap,
                meshlet_buffer=gs.meshlets, draw_commands_buffer=draw, material_buffer=gs.materials, draw_capacity=draw_cap,
                visibility_buffer=e_d, meshlet_visibility_buffer=m_d, material_count=material_count, **pyramid_kw)

    def reset():
        disp.zero_(), draw.zero_()
        e_d.copy_(dev(torch, evis)), m_d.copy_(dev(torch, mvis))
    return view, (lambda: (host(disp), host(draw), host(e_d, np.uint32), host(m_d, np.uint32))), reset


LATE = ["persp_256x16", "ortho_16x256", "persp_2x128"]


@pytest.mark.parametrize("cull_path", [1, 2], ids=["launch_chain", "one_launch"])
def test_cull_views_late_views_on_their_own_level_tables(torch_mod, oracle, cull_path):
    """orbit_cull_views with three late views (perspective and orthographic), each against its own per-mip images."""
    torch = torch_mod
    eng = make_engine("meshlet_buffer", max_views=3, cull_path=cull_path)
    cases = [gpu_case(torch, oracle, n) for n in LATE]
    views = [_view(torch, c, "random_words_materials", c["levels"].kw()) for c in cases]
    eng.cull_views([v for v, _, _ in views])
    torch.cuda.synchronize()
    eng.status()
    for c, (_, out, _) in zip(cases, views):
        assert_same(out(), reference(oracle, c, "random_words_materials"))
        c["levels"].check(c["pyr"])
    assert eng.fused_culls() == (3 if cull_path == 2 else 0)
    eng.close()


@pytest.mark.parametrize("cull_path", [1, 2], ids=["launch_chain", "one_launch"])
def test_frame_late_reduces_into_the_levels_its_late_views_read(torch_mod, oracle, cull_path):
    """orbit_frame_late: chain A writes the per-mip images (orbit_depth_reduce_multi) and the late views sample the same
    tables in the same call — eagerly, then captured and replayed as a graph."""
    torch = torch_mod
    eng = make_engine("meshlet_buffer", max_views=5, cull_path=cull_path)
    cases = [gpu_case(torch, oracle, n) for n in LATE[:2]]
    made = [reduced_levels(torch, eng, c, reduce=False) for c in cases]
    views = [_view(torch, c, "zero_words", lv.kw()) for c, (lv, _, _) in zip(cases, made)]
    f, keep = eng.prepare_frame_late(pyramids=[item for _, item, _ in made], late_views=[v for v, _, _ in views])

    def check(what):
        torch.cuda.synchronize()
        eng.status()
        for c, (lv, _, _), (_, out, _) in zip(cases, made, views):
            lv.check(c["pyr"])
            assert_same(out(), reference(oracle, c, "zero_words"))

    def reset():
        for (lv, _, _), (_, _, rs) in zip(made, views):
            rs()
            for t, _, w, h, _ in lv.images:
                t[1:h + 1, :w] = -7.0

    eng.frame_late(f)
    check("eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.frame_late(f)
    for rep in range(2):
        reset()
        g.replay()
        check(f"replay {rep}")
    assert eng.fused_culls() >= 2 if cull_path == 2 else eng.fused_culls() == 0
    del keep
    eng.close()
