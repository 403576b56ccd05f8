"""GPU tests of meshlet streams that start past meshlet 0 (tests/stream_windows.py: the windows, scripts, high and large
cases): the derived arrays, read back array by array after every step (orbit_meshlet_stream_read_arrays, _block_bounds),
against the NumPy model of tests/stream_ref.py, byte for byte; and the culls that read them — pass 0 per meshlet and per
block, under three alpha filters and two grid caps, the record lists and their expansion, a stream shorter than its draws
— against the oracle's commands for the window's draws.

After every step orbit_meshlet_stream_validate is run as well, and held to stream_windows.mirrors(): a clean status
where the stream holds, over its hull, what its source buffer holds; ORBIT_E_STALE — not a clean status — at the steps
where it cannot: the open gap of script (c), the first pass of script (b) while pieces are missing, a rewrite of script
(e) before its update.  (A second small model beside tests/stream_ref.py: the per-meshlet arrays against the buffer's
re-layout, and "every meshlet of the hull derived from the current source".)"""
import contextlib
import dataclasses

import numpy as np
import pytest

import stream_windows as sw
from orbit_amd import _lib, layouts as L
from stream_ref import assert_views_equal
from test_block_pretest_cpu import BOUND
from test_gpu_parity import dev, host, run_oracle, torch_mod  # noqa: F401

pytestmark = pytest.mark.gpu

ALPHAS = (L.ALPHA_ALL, L.ALPHA_OPAQUE | L.ALPHA_MASKED, L.ALPHA_TRANSPARENT)


@pytest.fixture(scope="module")
def engine(torch_mod):  # noqa: F811
    from orbit_amd.engine import Engine

    e = Engine(0, max_entities=4096, max_dispatches=16_384, max_draws=131_072)
    yield e
    e.close()


class DeviceWindow:
    """A window's two source buffers (guards around the Meshlets), its stream — created without an update — and the
    material tables of its scripts on the device."""

    def __init__(self, torch, engine, w, meshlets=None, tables=None):
        from orbit_amd.engine import MeshletStream

        self.torch, self.engine, self.w = torch, engine, w
        self.host = sw.window_buffer(w, meshlets)
        self.bufs = {k: dev(torch, self.host) for k in "AB"}
        self.base = {k: t.data_ptr() + 32 * sw.GUARD - 32 * w.first for k, t in self.bufs.items()}
        self.ms = MeshletStream(engine, None, w.first, w.capacity, initial_update=False)
        self.tables = {k: (dev(torch, t), n, t) for k, (t, n) in
                       (tables or {k: sw.materials(w, k) for k in ("M0", "M1")}).items()}
        self.materials = None  # key of the table the classes mirror
        self.source = None

    def apply(self, st, meshlets):
        if st[0] == "update":
            self.ms.update(self.base[st[1]], st[2], st[3])
            self.source = st[1]
        elif st[0] == "materials":
            self.materials = st[1]
            if st[1] is None:
                self.ms.set_materials(None, 0)
            else:
                self.ms.set_materials(self.tables[st[1]][0], self.tables[st[1]][1])
        else:  # an in-place rewrite reaches both buffers
            self.host[sw.GUARD:sw.GUARD + len(meshlets)] = meshlets
            for t in self.bufs.values():
                t.copy_(dev(self.torch, self.host))

    def material_buffer(self):
        return None if self.materials is None else self.tables[self.materials][0]

    def read(self):
        got = self.ms.read_arrays()
        w = self.w
        got["blk"] = np.zeros(((w.first + w.capacity - 1) >> 5) - (w.first >> 5) + 1, dtype=BOUND)
        _lib.check(self.engine._lib.orbit_meshlet_stream_block_bounds(self.engine._ctx, self.ms._h, w.first >> 5, len(got["blk"]),
                                                                      got["blk"].ctypes.data, None), self.engine._ctx)
        return got

    def check(self, ref, meshlets, what):
        """Arrays == reference, and validate says what the reference says of the buffer: clean where the stream holds
        what the buffer holds over its hull, ORBIT_E_STALE where it does not (a gap no update reached yet, a rewrite
        whose update is still to come)."""
        self.torch.cuda.synchronize()
        assert_views_equal(self.read(), ref.views(), what)
        if self.source is not None:
            self.ms.validate(self.base[self.source], self.material_buffer())
            if sw.mirrors(ref, meshlets):
                self.engine.status()
            else:
                with pytest.raises(_lib.OrbitError) as err:
                    self.engine.status()
                assert err.value.code == _lib.E_STALE, what

    def assert_untouched(self):
        for k, t in self.bufs.items():
            assert host(t).tobytes() == self.host.tobytes(), f"source buffer {k} (guards included) was written"

    def release(self):
        """The engine as the next test expects it, whatever happened in this one."""
        self.engine.set_block_cull(True)
        self.engine.set_block_cull_grid(0)
        self.engine.bind_meshlet_stream(None)
        self.ms.close()


@contextlib.contextmanager
def played(torch, engine, w, script, plan=None, **kw):
    """Runs `script` (or the steps of `plan`) on the library and the reference side by side, checking after every step
    -> (device, ref, meshlets) for the body; behind it the source buffers, guards included, must be as uploaded.  The
    stream is unbound and destroyed and the engine's block-path settings restored whether or not the body passes."""
    d = DeviceWindow(torch, engine, w, **kw)
    try:
        d.check(sw.StreamRef(w.first, w.capacity), None, f"{w.name} / {script} / created")  # zero-filled, class 3, no bounds
        ref = m = None
        for i, (st, ref, m) in enumerate(sw.replay(w, script, meshlets=kw.get("meshlets"), tables=kw.get("tables"), plan=plan)):
            d.apply(st, m)
            d.check(ref, m, f"{w.name} / {script} / step {i} {st}")
        yield d, ref, m
        d.assert_untouched()
    finally:
        d.release()


ARRAY_CASES = [(w, s) for w in sw.windows() + sw.high_windows() for s in sw.SCRIPTS if sw.applies(w, s)]


@pytest.mark.parametrize("w,script", ARRAY_CASES, ids=[f"{w.name}-{s}" for w, s in ARRAY_CASES])
def test_arrays_after_every_step(torch_mod, engine, w, script):
    with played(torch_mod, engine, w, script):
        pass


def test_arrays_of_the_large_stream(torch_mod, engine):
    """2^21 + 101 meshlets from meshlet 59, script (a): one whole update, then the materials — checked after each step like
    every window.  The build, bounds and validate launches of the first step and the classes and validate launches of the
    second all take a second round of their 8192-workgroup grid, and nothing runs behind a step before it is compared:
    what the second rounds wrote (meshlets from 2^21 on, blocks from 65537 on) is what the comparison reads."""
    F, C = sw.LARGE_FIRST, sw.LARGE_CAPACITY
    m = sw.large_meshlets()
    w = dataclasses.make_dataclass("Large", ["name", "first", "capacity"])("large", F, C)
    tables = {"L": (sw.large_materials(), 300)}
    plan = [("update", "A", F, C), ("materials", "L")]
    with played(torch_mod, engine, w, "a", plan=plan, meshlets=m, tables=tables) as (_, ref, _):
        v = ref.views()
        tail = slice((F + (1 << 21)) // 32 - (F >> 5), None)  # the blocks of the launches' second rounds
        assert 0 < np.unpackbits(v["link"].view(np.uint8)).sum() < C and v["blk"]["valid"][tail].any()
        assert len(set(ref.cls.tolist())) == 4 and len(set(ref.cls[(1 << 21) - F:].tolist())) >= 2, "classes of both planes"


def _bits(words, word0, lo, n):
    """Bits of global meshlets [lo, lo + n) out of `words`, whose first word is word `word0`."""
    return np.unpackbits(words.view(np.uint8), bitorder="little")[lo - 32 * word0:lo - 32 * word0 + n]


def test_read_arrays_of_inner_sub_ranges(torch_mod, engine):
    """orbit_meshlet_stream_read_arrays' own offsets: sub-ranges that begin and end inside words, on a word boundary, of
    one meshlet and of none, against slices of the read of the whole (unaligned) stream."""
    w = sw.window("a32_59_to_0")
    with played(torch_mod, engine, w, "a") as (d, _, _):
        F, C = w.first, w.capacity
        whole = d.ms.read_arrays()
        assert whole["sphere"].any() and whole["link"].any() and not (whole["cls0"] == 0xFFFFFFFF).all()
        for lo, n in ((F + 37, 200), (F + 1, 1), ((F | 31) + 1, 64), ((F | 31) + 32, 33), (F + C - 70, 70), (F + 5, 0)):
            assert F <= lo and lo + n <= F + C
            got = d.ms.read_arrays(lo, n)
            for k in ("sphere", "cone", "mat", "cmd", "cnt"):
                assert np.array_equal(got[k], whole[k][lo - F:lo - F + n]), (k, lo, n)
            words = ((lo + n - 1) >> 5) - (lo >> 5) + 1 if n else 0
            for k in ("link", "cls0", "cls1"):
                assert len(got[k]) == words
                assert np.array_equal(_bits(got[k], lo >> 5, lo, n), _bits(whole[k], F >> 5, lo, n)), (k, lo, n)
            at32 = [g for g in range(lo, lo + n) if g % 32 == 0]
            assert len(got["base32"]) == words
            for g in at32:
                assert np.array_equal(got["base32"][(g >> 5) - (lo >> 5)], whole["base32"][(g >> 5) - (F >> 5)]), (g, lo, n)


# ------------------------------------------------------------------------------------------------------------- culls
_scene_dev = {}


def scene_buffers(torch, key):
    if key not in _scene_dev:
        s = sw.scene(key)
        _scene_dev[key] = (dev(torch, s.entity_draw_buffer()), dev(torch, s.entities))
    return _scene_dev[key]


def expected_commands(oracle, w, ref, alpha, table):
    """The oracle's commands for the window's draws, of the scene as the STREAM holds it: the window's meshlets rebuilt
    from the reference's arrays (a never-derived meshlet is an empty one), the materials of the cull."""
    s = w.scene
    meshlets = s.meshlets.copy()
    meshlets[w.m0:w.m1] = sw.stream_meshlets(ref)
    out = run_oracle(oracle, dataclasses.replace(s, meshlets=meshlets, materials=table), sw.cull_info(w.key, alpha))
    assert out[4] == 0 and out[5] == 0
    return w.commands(L.draw_buffer_commands(out[1])[1])


def cull(torch, engine, w, d, alpha, mesh_infos, records=False):
    """entity_cull of the window's draws and meshlet_cull on the shifted base -> commands (through the record list and its
    expansion with `records`)."""
    s = w.scene
    draws, entities = scene_buffers(torch, w.key)
    ci = sw.cull_info(w.key, alpha)
    cap_d, cap_c = s.max_dispatches() + 8, s.lod0_meshlets + 8
    disp = torch.full((L.DISPATCH_HEADER + 16 * cap_d + 256,), 0xAB, dtype=torch.uint8, device="cuda")
    draw = torch.full((L.DRAW_HEADER + 28 * cap_c + 256,), 0xCD, dtype=torch.uint8, device="cuda")
    base, mat = d.base[d.source], d.material_buffer()
    engine.entity_cull(ci, draws, mesh_infos, disp, entities, w.e - w.b, cap_d, draw_first=w.b)
    if records:
        vis = torch.full((L.VISIBLE_HEADER + 12 * cap_d + 256,), 0xCD, dtype=torch.uint8, device="cuda")
        engine.meshlet_cull_visible_records(ci, disp, base, vis, entities, mat, cap_d, cap_d)
        engine.expand_visible_records(vis, base, draw, cap_c)
    else:
        engine.meshlet_cull(ci, disp, base, draw, entities, mat, cap_d, cap_c)
    torch.cuda.synchronize()
    assert bool((disp[L.DISPATCH_HEADER + 16 * cap_d:] == 0xAB).all()) and bool((draw[L.DRAW_HEADER + 28 * cap_c:] == 0xCD).all())
    return L.draw_buffer_commands(host(draw))[1]


def culls_every_way(torch, engine, oracle, w, d, ref, classes=True):
    """Block path on and off, three alpha filters, grid caps 0 and 1: the oracle's commands, a clean status, and the
    counters of test_block_cull_gpu.both_ways (`classes` False: the stream holds a class-3 meshlet, neither advances)."""
    mesh_infos = dev(torch, w.mesh_infos())
    table = d.tables[d.materials][2]
    engine.bind_meshlet_stream(d.ms)
    total = 0
    try:
        for alpha in ALPHAS:
            want = expected_commands(oracle, w, ref, alpha, table)
            total += len(want)
            for on, cap in ((True, 0), (True, 1), (False, 0)):
                engine.set_block_cull(on)
                engine.set_block_cull_grid(cap)
                before = engine.block_culls(), engine.meshlet_class_culls(), engine.meshlet_stream_culls()
                got = cull(torch, engine, w, d, alpha, mesh_infos)
                engine.status()
                what = f"{w.name}, alpha {alpha}, block path {on}, cap {cap}"
                assert len(got) == len(want) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), what
                assert engine.meshlet_stream_culls() == before[2] + 1, what
                assert engine.meshlet_class_culls() == before[1] + (1 if classes else 0), what
                assert engine.block_culls() == before[0] + (1 if on and classes else 0), what
    finally:
        engine.set_block_cull(True)
        engine.set_block_cull_grid(0)
        engine.bind_meshlet_stream(None)
    assert total > 0, "the window draws something under some filter"


CULL_WINDOWS = sw.windows() + sw.high_windows()


@pytest.mark.parametrize("w", CULL_WINDOWS, ids=repr)
def test_culls_after_a_whole_update(torch_mod, engine, oracle, w):
    with played(torch_mod, engine, w, "a") as (d, ref, _):
        culls_every_way(torch_mod, engine, oracle, w, d, ref)


@pytest.mark.parametrize("script", ["b", "c", "e"])
@pytest.mark.parametrize("name", ["a32_59_to_0", "ragged_32_mid"])
def test_culls_after_pieces_a_gap_and_rewrites(torch_mod, engine, oracle, name, script):
    """(c) leaves its gap open: the stream holds empty meshlets there, with the class of material 0 and — where a block
    is partly derived — bounds that include their zero spheres; the culls draw what the oracle draws of that scene."""
    w = sw.window(name)
    with played(torch_mod, engine, w, script) as (d, ref, _):
        culls_every_way(torch_mod, engine, oracle, w, d, ref)


@pytest.mark.parametrize("name", ["a32_63_to_63", "ragged2_head"])
def test_culls_with_a_class_3_meshlet_read_the_indices(torch_mod, engine, oracle, name):
    w = sw.window(name)
    with played(torch_mod, engine, w, "f") as (d, ref, m):
        t, count = sw.materials(w, "M1")
        assert (m["material_index"] >= count).any() and (t["alpha_mode"][m["material_index"]] == 3).any()
        culls_every_way(torch_mod, engine, oracle, w, d, ref, classes=False)


@pytest.mark.parametrize("name", ["a32_59_to_0", "high_ends_at_FFFFFFFF"])
def test_record_lists_and_their_expansion(torch_mod, engine, oracle, name):
    w = sw.window(name)
    with played(torch_mod, engine, w, "a") as (d, ref, _):
        engine.bind_meshlet_stream(d.ms)
        before = engine.meshlet_stream_culls()
        got = cull(torch_mod, engine, w, d, L.ALPHA_ALL, dev(torch_mod, w.mesh_infos()), records=True)
        engine.status()
        assert engine.meshlet_stream_culls() == before + 2  # the cull and the expansion
        want = expected_commands(oracle, w, ref, L.ALPHA_ALL, d.tables["M0"][2])
        assert len(want) > 0 and len(got) == len(want) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_stream_shorter_than_its_draws(torch_mod, engine, oracle):
    """test_block_pipeline_gpu.test_range_status with first != 0: the records of the window's last two draws lie behind the
    stream — not read, ORBIT_E_RANGE, the same list and the same text with the block path on and off; the draws in front
    of them are drawn as the oracle draws them."""
    torch = torch_mod
    w = sw.short_window()
    with played(torch, engine, w, "a") as (d, ref, _):
        mesh_infos = dev(torch, w.mesh_infos())
        engine.bind_meshlet_stream(d.ms)
        out = []
        for on in (True, False):
            engine.set_block_cull(on)
            before = engine.block_culls()
            got = cull(torch, engine, w, d, L.ALPHA_ALL, mesh_infos)
            assert engine.block_culls() == before + (1 if on else 0)
            with pytest.raises(_lib.OrbitError) as err:
                engine.status()
            assert err.value.code == _lib.E_RANGE
            out.append((got, str(err.value)))
        assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and out[0][1] == out[1][1]
        want = expected_commands(oracle, w, ref, L.ALPHA_ALL, d.tables["M0"][2])
        inside = out[0][0][out[0][0]["cmd_first_instance"] < w.e - 2]
        want = want[want["cmd_first_instance"] < w.e - 2]
        assert len(want) > 0 and np.array_equal(inside.view(np.uint32), want.view(np.uint32))
