"""orbit_cluster_stats on the CPU: the OrbitClusterStats layout in the header, the ctypes dtype and the Rust binding; the
numpy statement (tests/cluster_stats_ref.py) against the oracle's mark, compaction and assignment and against
np_restatement's uncapped counts on every golden cluster case; the documented invariants."""
import os
import re

import numpy as np
import pytest

import cluster_stats_ref as ref
import np_restatement as npr
from orbit_amd import layouts as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = list(L.CLUSTER_STATS_SCALARS) + ["reserved0", "clusters_by_lights", "reserved1", "samples_by_lights", "reserved2"]


def test_header_layout_and_static_asserts():
    text = open(os.path.join(ROOT, "include", "orbit_abi_ext.h")).read()
    body = re.search(r"typedef struct OrbitClusterStats \{(.*?)\} OrbitClusterStats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"uint64_t\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [n for n, _ in names] == FIELDS
    assert sum(int(k or 1) for _, k in names) == 32  # 256 B of u64
    for want in ("sizeof(OrbitClusterStats) == 256", "offsetof(OrbitClusterStats, sample_light_refs) == 48",
                 "offsetof(OrbitClusterStats, clusters_by_lights) == 64",
                 "offsetof(OrbitClusterStats, samples_by_lights) == 128", "offsetof(OrbitClusterStats, reserved2) == 168"):
        assert f"ORBIT_STATIC_ASSERT({want}" in text, want
    assert "int32_t orbit_cluster_stats(" in text


def test_ctypes_dtype_and_rust_struct():
    assert L.CLUSTER_STATS.itemsize == 256 and list(L.CLUSTER_STATS.names) == FIELDS
    off = {n: L.CLUSTER_STATS.fields[n][1] for n in FIELDS}
    assert (off["sample_light_refs"], off["clusters_by_lights"], off["samples_by_lights"], off["reserved2"]) == (48, 64, 128, 168)
    rust = open(os.path.join(ROOT, "bindings", "rust", "orbit_hip.rs")).read()
    body = re.search(r"pub struct OrbitClusterStats \{(.*?)\}", rust, re.S).group(1)
    fields = re.findall(r"pub (\w+): (u64|\[u64; (\d+)\])", body)
    assert [f[0] for f in fields] == FIELDS
    assert sum(int(f[2] or 1) for f in fields) == 32


def test_light_classes_at_their_bounds():
    got = ref.light_class([0, 1, 16, 17, 64, 65, 255, 256, 257, 10_000]).tolist()
    assert got == [0, 1, 1, 2, 2, 3, 3, 3, 4, 4]
    assert [lo for lo, _ in L.CLUSTER_STATS_CLASSES] == [0, 1, 17, 65, 257]


def test_stats_dict_reads_the_layout():
    from orbit_amd.engine import cluster_stats_dict

    raw = np.arange(32, dtype=np.uint64)
    d = cluster_stats_dict(raw)
    assert d["samples"] == 0 and d["sample_light_refs"] == 6
    assert d["clusters_by_lights"] == [8, 9, 10, 11, 12] and d["samples_by_lights"] == [16, 17, 18, 19, 20]
    assert not any(k.startswith("reserved") for k in d)


@pytest.mark.parametrize("case", ref.CASES)
def test_restated_slices_reproduce_the_oracle_mark(oracle, case):
    c = ref.load_case(case)
    om, ob = oracle.cluster_mark(c["push"], c["depth"])
    rm, rb = ref.mark(c["push"], c["depth"])
    assert np.array_equal(rm, om), "tile slice masks differ"
    assert np.array_equal(rb, ob.reshape(-1, 2)), "depth bounds differ"


@pytest.mark.parametrize("case", ref.CASES)
def test_counts_against_the_restatement_and_the_oracle(oracle, case):
    c = ref.load_case(case)
    s, (active, n_samples, count) = ref.stats(c["push"], c["info"], c["depth"], c["lights"])
    ref.check_invariants(s)
    cc = [int(v) for v in c["push"]["cluster_count"]]
    total = cc[0] * cc[1] * cc[2]
    om, ob = oracle.cluster_mark(c["push"], c["depth"])
    ou, dropped = oracle.cluster_compact(cc, om, total)
    na = int(ou[12:16].view(np.uint32)[0])
    assert dropped == 0 and na == s["active_clusters"]
    listed = ou[16:16 + 4 * na].view(np.uint32)
    assert np.array_equal(np.sort(listed), active), "active clusters differ from the compaction's"
    # np_restatement's uncapped counts, in list order
    nl = int(c["info"]["global_light_count"])
    _, _, ucount, _ = npr.cluster_assign(c["info"], ou, ob, c["lights"][:nl], 256 * na + 16, total)
    order = np.argsort(listed)
    assert np.array_equal(ucount[order], count), "uncapped counts differ from np_restatement.cluster_assign"
    # the oracle's capped image and light_count header
    ol, oimg, dropped = oracle.cluster_assign(c["info"], ou, ob, c["lights"], 256 * na + 16, total)
    assert dropped == 0
    assert np.array_equal(oimg[active, 1], np.minimum(count, 256)), "capped counts differ from the oracle's image"
    assert int(ol[:4].view(np.uint32)[0]) == s["light_indices"]
    assert s["sample_light_refs"] == int((n_samples * oimg[active, 1].astype(np.int64)).sum())


def test_the_cases_reach_the_cap_and_the_grid_edges():
    """What the GPU tests compare is only as good as the work the cases hold: a saturated cluster, a grid that does not
    reach past the screen, samples outside the grid, a case without lights."""
    seen = {}
    for case in ref.CASES:
        c = ref.load_case(case)
        seen[case] = ref.stats(c["push"], c["info"], c["depth"], c["lights"])[0]
    assert any(s["clusters_by_lights"][4] > 0 for s in seen.values())
    assert all(s["samples_outside_grid"] > 0 for s in seen.values())
    assert seen["spirv_cluster_shapes/t16_none"]["light_refs"] == 0
    assert sum(1 for s in seen.values() if s["clusters_by_lights"][2] + s["clusters_by_lights"][3] > 0) >= 2
