"""orbit_cull_stats on the CPU: the OrbitCullStats layout in the header, the ctypes dtype and the Rust binding; the numpy
classifier (tests/cull_stats_ref.py) against np_restatement's culls and the oracle on the scene set; the documented
invariants; and that the scene set gives every counter work."""
import os
import re

import numpy as np
import pytest

import cull_stats_ref as ref
import np_restatement as npr
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(L.CULL_STATS_ENTITY) + ["records", "reserved0", "lod_drawn"] + list(L.CULL_STATS_MESHLET) + ["reserved1"]


def test_header_layout_and_static_asserts():
    text = open(os.path.join(ROOT, "include", "orbit_abi_ext.h")).read()
    body = re.search(r"typedef struct OrbitCullStats \{(.*?)\} OrbitCullStats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"uint64_t\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [n for n, _ in names] == FIELDS
    assert sum(int(k or 1) for _, k in names) == 32  # 256 B of u64
    for want in ('sizeof(OrbitCullStats) == 256', 'offsetof(OrbitCullStats, records) == 48',
                 'offsetof(OrbitCullStats, lod_drawn) == 64', 'offsetof(OrbitCullStats, meshlets) == 128',
                 'offsetof(OrbitCullStats, meshlet_drawn) == 184', 'offsetof(OrbitCullStats, reserved1) == 192'):
        assert f"ORBIT_STATIC_ASSERT({want}" in text, want
    assert "int32_t orbit_cull_stats(" in text


def test_ctypes_dtype_and_rust_struct():
    assert L.CULL_STATS.itemsize == 256 and list(L.CULL_STATS.names) == FIELDS
    off = {n: L.CULL_STATS.fields[n][1] for n in FIELDS}
    assert (off["records"], off["lod_drawn"], off["meshlets"], off["meshlet_drawn"], off["reserved1"]) == (48, 64, 128, 184, 192)
    rust = open(os.path.join(ROOT, "bindings", "rust", "orbit_hip.rs")).read()
    body = re.search(r"pub struct OrbitCullStats \{(.*?)\}", rust, re.S).group(1)
    fields = re.findall(r"pub (\w+): (u64|\[u64; (\d+)\])", body)
    assert [f[0] for f in fields] == FIELDS
    assert sum(int(f[2] or 1) for f in fields) == 32


def test_stats_dict_helper():
    from orbit_amd.engine import cull_stats_dict

    d = cull_stats_dict(np.arange(32, dtype=np.uint64))
    assert d["entities"] == 0 and d["records"] == 6 and d["lod_drawn"] == list(range(8, 16))
    assert d["meshlets"] == 16 and d["meshlet_drawn"] == 23 and not any(k.startswith("reserved") for k in d)


@pytest.fixture(scope="module")
def classified(oracle):
    return {name: (c, ref.classify_case(c)) for name in ref.CASES for c in [ref.make_case(name, oracle)]}


@pytest.mark.parametrize("name", ref.CASES)
def test_classifier_agrees_with_the_restatement_and_the_oracle(oracle, classified, name):
    c, got = classified[name]
    s = c["scene"]
    ref.check_invariants(got)
    # entity stage: np_restatement's drawn set and records, and the oracle's
    _, should, recs_n, _ = npr.entity_cull(c["ci"], s.entity_draws, c["count"], c["edc"], s.mesh_infos, s.entities,
                                           c["evis"], c["pyr"], c["psize"])
    assert got["entity_drawn"] == int(should.sum())
    assert np.array_equal(got["_records"].view(np.uint32), recs_n.view(np.uint32))
    cap_d = len(recs_n) + 8
    disp, _, dropped = oracle.entity_cull(c["ci"], s.entity_draw_buffer(c["count"]), c["edc"], s.mesh_infos, s.entities,
                                          cap_d, c["evis"], c["pyr"], c["psize"])
    hdr, orecs = L.dispatch_buffer_records(disp)
    assert dropped == 0 and int(hdr[0]) == got["records"]
    assert np.array_equal(orecs.view(np.uint32), got["_records"].view(np.uint32))
    # meshlet stage over those records: the drawn meshlets, in command order, are np_restatement's and the oracle's
    cmds_n, _ = npr.meshlet_cull(c["ci"], recs_n, s.meshlets, s.entities, s.materials, c["mvis"], c["pyr"], c["psize"])
    assert got["meshlet_drawn"] == len(cmds_n)
    lane = np.tile(np.arange(npr.S), len(recs_n))
    rid = np.repeat(np.arange(len(recs_n)), npr.S)
    act = lane < recs_n["meshlet_count"][rid]
    idx = (recs_n["meshlet_offset"][rid] + lane)[act]
    assert np.array_equal(idx[got["_meshlet_drawn"]], cmds_n["meshlet_index"])
    draw, _, dropped = oracle.meshlet_cull(c["ci"], disp, s.meshlets, got["meshlets"] + 8, s.entities, s.materials,
                                           c["mvis"], c["pyr"], c["psize"])
    n, ocmds = L.draw_buffer_commands(draw)
    assert dropped == 0 and n == got["meshlet_drawn"]
    assert np.array_equal(ocmds["meshlet_index"], cmds_n["meshlet_index"])
    assert got["meshlets"] == int(recs_n["meshlet_count"].sum())


def test_every_counter_has_work_in_the_scene_set(classified):
    """Asserted on the host before any GPU comparison leans on it: each class, each LOD slot, is non-zero somewhere."""
    totals = {}
    for _, got in classified.values():
        for k, v in ref.public(got).items():
            if k == "lod_drawn":
                for i, x in enumerate(v):
                    totals[f"lod_drawn[{i}]"] = totals.get(f"lod_drawn[{i}]", 0) + x
            else:
                totals[k] = totals.get(k, 0) + v
    empty = sorted(k for k, v in totals.items() if v == 0)
    assert not empty, empty
    # the pass-2 override: with noskip_alphamode unset the alpha flag is ignored, with it set the flag decides
    _, p2 = classified["p2_persp"]
    _, p2n = classified["p2_persp_noskip"]
    assert p2["meshlet_alpha_filtered"] == 0 and p2["meshlet_drawn_in_early_pass"] > 0
    assert p2n["meshlet_alpha_filtered"] > 0


def test_invariants_hold_on_a_capacity_independent_count(oracle, classified):
    """The counters are uncapped: the oracle cut to half its capacity drops records, the classifier does not."""
    c, got = classified["p0_persp_lods"]
    s = c["scene"]
    cap = got["records"] // 2
    disp, _, dropped = oracle.entity_cull(c["ci"], s.entity_draw_buffer(), c["edc"], s.mesh_infos, s.entities, cap)
    assert dropped > 0 and int(L.dispatch_buffer_records(disp)[0][0]) == cap < got["records"]
