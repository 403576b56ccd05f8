"""The pass-2 HiZ test at its edges, CPU side (tests/hiz_edges.py): the hostile cases exercise what they are for (a
census of the reference side alone), the C oracle equals the numpy restatement on every one of them, and it equals
the reference's own binaries on the committed ones (tests/golden/spirv_cull_hiz_edges.npz), in both arithmetic
profiles.  tests/test_hiz_edges_gpu.py runs the same cases through every kernel path."""
import os

import numpy as np
import pytest

import hiz_edges as hz
from orbit_amd import layouts as L
from test_oracle_cpu import _run_both
from test_spirv_vectors_cpu import load_case

ALL = list(hz.CASES) + list(hz.VECTOR_CASES)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spirv_cull_hiz_edges.npz")
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")  # numpy's, on the non-finite inputs these cases are made of
OUTPUTS = ("spv_dispatch", "spv_draw", "spv_evis", "spv_mvis", "spv_task_records", "spv_task_mvis")


def _drawn(oracle, c, pyr):
    s = c["scene"]
    evis, mvis = hz.words(s, "zero")
    disp, _, d1 = oracle.entity_cull(c["ci"], s.entity_draw_buffer(), s.entity_draw_count, s.mesh_infos, s.entities,
                                     s.max_dispatches() + 8, evis, pyr, c["psize"])
    draw, _, d2 = oracle.meshlet_cull(c["ci"], disp, s.meshlets, s.lod0_meshlets + 8, s.entities, s.materials, mvis, pyr,
                                      c["psize"])
    assert d1 == 0 and d2 == 0
    cmds = L.draw_buffer_commands(draw)[1]
    return {(int(a), int(b)) for a, b in zip(cmds["cmd_first_instance"], cmds["meshlet_index"])}


@pytest.mark.parametrize("name", ALL)
def test_census_floors(oracle, name):
    """A condition on the INPUTS, taken from the numpy restatement's intermediates: every class a case can show has at
    least 4 rows in the entity stage and 64 in the meshlet stage among the rows that reach the occlusion test, both
    stages decide both ways, and the HiZ test removes some but not all of what is drawn against a pyramid that
    occludes nothing (every texel -inf).  The classes a case cannot show carry their reason (hiz_edges.unreachable)."""
    c = hz.make_case(name, oracle)
    ce, cm, recs, cmds = hz.take_census(c)
    un = hz.unreachable(c)
    assert all(reason for reason in un.values())
    short = {f"{stage}:{k}": v for stage, cen, floor in (("entity", ce, 4), ("meshlet", cm, 64))
             for k, v in cen.items() if k not in un and v < floor}
    assert not short, short
    assert {f"level_{k}" for k in range(c["mips"])} <= set(cm) and len(cmds) > 0
    if max(c["psize"]) >= 64 and not c["floor"]:  # the planted blocks are all there: no sampled class is excused
        assert not {"sampled_nan", "sampled_pinf", "sampled_ninf", "sampled_negative"} & set(un)
    for cen in (ce, cm):  # both outcomes (among finite rows: the floors above; here among all that sample)
        assert cen["finite_visible"] > 0 and cen["finite_culled"] > 0
    with_hiz, without = _drawn(oracle, c, c["pyr"]), _drawn(oracle, c, np.full_like(c["pyr"], -np.inf))
    assert with_hiz and with_hiz < without


@pytest.mark.parametrize("words", ["zero", "random"])
@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_numpy_restatement_on_the_hostile_cases(oracle, name, words):
    """Two restatements by different means agree bit for bit — on records, commands and both bitsets — which pins the
    sampler MODEL (level selection, footprint clamps, the min over non-finite texels) that the binaries do not hold."""
    c = hz.make_case(name, oracle)
    evis, mvis = hz.words(c["scene"], words, seed=3)
    recs, cmds, _, _ = _run_both(oracle, c["scene"], c["ci"], evis, mvis, c["pyr"], c["psize"])
    assert len(recs) > 100 and len(cmds) > 100


# ------------------------------------------------------------------------------- the reference's binaries on such cases
@pytest.fixture(scope="module")
def vectors():
    return np.load(GOLD)


def load_contracted(vectors, name):
    c = load_case(vectors, name)
    for k in OUTPUTS:
        c[k] = vectors[f"{name}/contracted/{k}"]
    c["spv_task_records"] = c["spv_task_records"].view(L.MESH_TASK_RECORD)
    return c


def test_the_committed_cases_are_the_helpers(oracle, vectors):
    """The file's inputs are hiz_edges.VECTOR_CASES (so the census floors above speak about them): perspective and
    orthographic, no cull planes, the pyramids 256x128, 256x16, 16x256 and 1x1."""
    assert {n.split("/")[0] for n in vectors.files} == set(hz.VECTOR_CASES)
    assert {tuple(int(v) for v in vectors[f"{n}/pyramid_size"]) for n in hz.VECTOR_CASES} == {
        (256, 128), (256, 16), (16, 256), (1, 1)}
    assert {int(load_case(vectors, n)["ci"]["projection_type"]) for n in hz.VECTOR_CASES} == {0, 1}
    for name in hz.VECTOR_CASES:
        c, v = hz.make_case(name, oracle), load_case(vectors, name)
        assert int(v["ci"]["occlusion_pass"]) == 2 and int(v["ci"]["cull_plane_count"]) == 0
        assert np.array_equal(v["pyr"].view(np.uint32), c["pyr"].view(np.uint32))
        assert v["meshlets"].tobytes() == c["scene"].meshlets.tobytes()
        assert v["entities"].tobytes() == c["scene"].entities.tobytes()
        assert v["mesh_infos"].tobytes() == c["scene"].mesh_infos.tobytes()


@pytest.mark.parametrize("profile", [0, 1], ids=["canonical", "contracted"])
@pytest.mark.parametrize("name", list(hz.VECTOR_CASES))
def test_oracle_equals_the_reference_binaries_on_the_hostile_cases(oracle, vectors, name, profile):
    """entity_cull.comp.spv, meshlet_cull.comp.spv and forward_depth_prepass.task.spv, executed by oracle/spirv_vm.py on
    hostile geometry against hostile pyramids, canonical and with Dot / matrix products / Length as fma chains: dispatch
    records, commands, both visibility bitsets, the task records and the words the task stage writes.
    The ReduceMin sampler is NOT in the binaries — the interpreter calls oracle.hiz_sample — so this pins the arithmetic
    up to the sample (the sphere's projection from degenerate and non-finite input, lod, closest, the comparison, the
    bit protocol); the sampler model itself is pinned by the independent numpy restatement above."""
    c = load_contracted(vectors, name) if profile else load_case(vectors, name)
    n_draws = int(np.frombuffer(c["draws"][:4].tobytes(), np.uint32)[0])
    pk = (c["pyr"], c["ps"])
    with oracle.arith_profile(profile):
        od, oev, dropped = oracle.entity_cull(c["ci"], c["draws"], n_draws, c["mesh_infos"], c["entities"], c["caps"][0],
                                              c["evis"], *pk)
        nrec = int(c["spv_dispatch"][:4].view(np.uint32)[0])
        assert dropped == 0 and int(od[:4].view(np.uint32)[0]) == nrec > 100
        assert np.array_equal(od[:L.DISPATCH_HEADER + 16 * nrec], c["spv_dispatch"]), "dispatch records differ from the binary's"
        oc, omv, dropped = oracle.meshlet_cull(c["ci"], od, c["meshlets"], c["caps"][1], c["entities"], c["materials"],
                                               c["mvis"], *pk)
        ndraw = int(c["spv_draw"][:4].view(np.uint32)[0])
        assert dropped == 0 and int(oc[:4].view(np.uint32)[0]) == ndraw > 100
        assert np.array_equal(oc[:L.DRAW_HEADER + 28 * ndraw], c["spv_draw"]), "draw commands differ from the binary's"
        assert np.array_equal(oev, c["spv_evis"]) and np.array_equal(omv, c["spv_mvis"]), "visibility words differ"
        recs, tmv = oracle.meshlet_task_cull(c["ci"], c["spv_dispatch"], c["meshlets"], c["entities"], c["materials"],
                                             c["mvis"], *pk)
        assert np.array_equal(recs.view(np.uint8), c["spv_task_records"].view(np.uint8)), "task records differ from the binary's"
        assert np.array_equal(tmv, c["spv_task_mvis"])
    assert oracle.lib().oracle_get_arith_profile() == 0
