"""The glb scene of the raster tests (tools/make_test_glb.py through the host mirror's ingestion) and the chains that
run on it on the CPU: the oracle's culls, the host mirror's raster (orbit_amd.raster.host_raster_depth), the oracle's
depth_reduce.  Shared by tests/test_raster_depth_cpu.py and tests/test_raster_depth_gpu.py; computed once per process."""
import functools
import importlib.util
import os
import tempfile

import numpy as np

import scenes as sc
from orbit_amd import gltf, raster
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GlbScene:
    def __init__(self, instances, seed=7):
        spec = importlib.util.spec_from_file_location("make_test_glb", os.path.join(ROOT, "tools", "make_test_glb.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        with tempfile.TemporaryDirectory() as tmp:
            glb = os.path.join(tmp, "scene.glb")
            tool.write(glb, instances=instances, seed=seed)
            b = gltf.to_scene_buffers(gltf.load(glb))
        self.entity_draws = np.ascontiguousarray(b["entity_draws"]).view(np.uint8).reshape(-1)
        self.mesh_infos, self.entities, self.meshlets = b["mesh_infos"], b["entities"], b["meshlets"]
        self.materials, self.meshlet_data = b["materials"], np.ascontiguousarray(b["meshlet_data"], np.uint32)
        self.vertices = np.ascontiguousarray(b["vertex_positions"], np.float32)
        self.n = int(self.entity_draws[:4].view(np.uint32)[0])
        draws = self.entity_draws[4:4 + 12 * self.n].view(L.ENTITY_DRAW)
        per_draw_max = self.mesh_infos["mesh_lods"][draws["mesh_index"]][:, :, 1].max(axis=1)
        self.cap_d, self.cap_c = int((per_draw_max // 32 + 1).sum()) + 8, int(per_draw_max.sum()) + 8
        self.vis_words = int(draws["visibility_offset"].max()) + int(per_draw_max.max()) // 32 + 2
        self.entity_count = len(np.ascontiguousarray(self.entities).view(np.uint8).reshape(-1)) // 128

    def cull(self, oracle, cam, occlusion_pass=0, planes=None, evis=None, mvis=None, pyramid=None, pyramid_size=(0, 0)):
        """The oracle's entity + meshlet cull -> (dispatch bytes, draw bytes, entity vis, meshlet vis)."""
        ci = sc.make_cull_info(cam.view, cam.planes if planes is None else planes, occlusion_pass=occlusion_pass,
                               p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
        disp, oev, dd = oracle.entity_cull(ci, self.entity_draws, self.n, self.mesh_infos, self.entities, self.cap_d,
                                           evis, pyramid, pyramid_size)
        draw, omv, dc = oracle.meshlet_cull(ci, disp, self.meshlets, self.cap_c, self.entities, self.materials, mvis,
                                            pyramid, pyramid_size)
        assert dd == 0 and dc == 0
        return ci, disp, draw, oev, omv

    def all_commands(self, oracle, cam):
        """Every non-transparent meshlet of the records the oracle's entity stage writes with ZERO planes (the LOD
        pick applied, nothing culled), as the draw commands meshlet_cull.comp would write for them."""
        ci = sc.make_cull_info(cam.view, np.zeros((0, 4), np.float32), p00=cam.p00, p11=cam.p11, z_near=cam.z_near)
        disp, _, dd = oracle.entity_cull(ci, self.entity_draws, self.n, self.mesh_infos, self.entities, self.cap_d)
        assert dd == 0
        _, recs = L.dispatch_buffer_records(disp)
        cmds = []
        for r in recs:
            for m in range(int(r["meshlet_offset"]), int(r["meshlet_offset"]) + int(r["meshlet_count"])):
                ml = self.meshlets[m]
                if int(self.materials[int(ml["material_index"])]["alpha_mode"]) == 2:
                    continue
                data_offset, nv, nt = int(ml["data_offset"]), int(ml["vertex_count"]), int(ml["triangle_count"])
                cmds.append((3 * nt, 1, (data_offset + nv) * 4, data_offset, int(r["entity_index"]), int(ml["vertex_offset"]), m))
        return raster.command_buffer(np.array(cmds, L.MESHLET_DRAW_COMMAND))

    def host_raster(self, draw_bytes, cam, width, height, depth=None, clear=True, max_commands=None):
        words = np.ascontiguousarray(draw_bytes).view(np.uint8).reshape(-1)
        max_commands = (words.nbytes - 4) // 28 if max_commands is None else max_commands
        return raster.host_raster_depth(words, max_commands, self.meshlet_data, self.vertices, len(self.vertices),
                                        self.entities, view_proj(cam), width, height, depth=depth, clear=clear)


def view_proj(cam):
    """proj x view, column-major float32[16], as the renderer hands it to the depth prepass."""
    return sc.mat4_cols((cam.proj.astype(np.float32) @ cam.view.astype(np.float32)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def glb_scene(instances, seed=7):
    return GlbScene(instances, seed)


def camera(width, height, position=(0.0, 1.0, 6.0), rot=(1.0, 0.0)):
    return sc.default_camera(position=position, rot=rot, aspect=width / height)


def two_pass_frame(scene, oracle, cam0, cam1, width, height):
    """Frame 0 from nothing at cam0, then the two-pass frame of forward.rs:266-429 at cam1, on the CPU: early cull with
    the previous frame's bits -> raster CLEAR -> depth_reduce -> late cull -> raster LOAD.  -> dict of every stage."""
    out = {}
    evis, mvis = np.zeros((scene.n + 31) // 32, np.uint32), np.zeros(scene.vis_words, np.uint32)
    for f, cam in enumerate((cam0, cam1)):
        _, _, draw1, _, _ = scene.cull(oracle, cam, 1, evis=evis, mvis=mvis)
        depth1, st1, err1 = scene.host_raster(draw1, cam, width, height)
        pyr, pd = oracle.depth_reduce(depth1, width, height)
        _, disp2, draw2, evis2, mvis2 = scene.cull(oracle, cam, 2, evis=evis, mvis=mvis, pyramid=pyr,
                                                   pyramid_size=(pd.width, pd.height))
        depth2, st2, err2 = scene.host_raster(draw2, cam, width, height, depth=depth1, clear=False)
        assert not err1.any() and not err2.any()
        out[f] = dict(evis_in=evis, mvis_in=mvis, draw1=draw1, depth1=depth1, stats1=st1, pyramid=pyr, pyramid_desc=pd,
                      draw2=draw2, depth2=depth2, stats2=st2, evis=evis2, mvis=mvis2)
        evis, mvis = evis2, mvis2
    return out


def hiz_rejected(scene, oracle, cam, frame):
    """Meshlets the late pass's HiZ test rejected: the late cull's survivors against the same cull with a pyramid of
    zeros (reversed z: nothing is behind depth 0, so nothing is occluded)."""
    pd = frame["pyramid_desc"]
    _, _, draw_open, _, _ = scene.cull(oracle, cam, 2, evis=frame["evis_in"], mvis=frame["mvis_in"],
                                       pyramid=np.zeros_like(frame["pyramid"]), pyramid_size=(pd.width, pd.height))
    return int(draw_open[:4].view(np.uint32)[0]) - int(frame["draw2"][:4].view(np.uint32)[0])
