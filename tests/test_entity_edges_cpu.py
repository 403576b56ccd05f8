"""The entity stage at its launch-form, chunk and range edges, CPU side (tests/entity_edges.py): the cases exercise what
they are for (a census of the reference side alone), the C oracle equals the numpy restatement on every one of them —
whole-buffer calls whose draw buffer claims fewer or more draws than the call is given included —, the oracle's range
calls add up to its whole call, and the table the case sizes are derived from is the source text's."""
import os
import re

import numpy as np
import pytest

import entity_edges as ee
import np_restatement as npr
from orbit_amd import layouts as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orbit_amd", "csrc")


def _restated(case, occlusion_pass, header, vis, S=32, profile=0, detail=None):
    """np_restatement.entity_cull of a whole-buffer call given N draws whose draw buffer's header says `header`."""
    s = case["scene"]
    return npr.entity_cull(ee.cull_info(case, occlusion_pass), s.entity_draws, header, case["n"], s.mesh_infos, s.entities,
                           vis, case["pyr"], case["psize"], detail=detail, S=S, contract=bool(profile))


def _oracle(oracle, case, occlusion_pass, header, vis, first=None, count=None, capacity=None):
    s = case["scene"]
    return oracle.entity_cull(ee.cull_info(case, occlusion_pass), ee.draw_buffer(case, header),
                              case["n"] if count is None else count, s.mesh_infos, s.entities,
                              case["capacity"] if capacity is None else capacity, vis, case["pyr"], case["psize"],
                              draw_first=first)


def _chunk_records(per_draw, n):
    """Records per chunk of 256 draws, over the first n draws."""
    padded = np.zeros(ee.chunks_of(n) * ee.CHUNK, np.int64)
    padded[:n] = per_draw[:n]
    return padded.reshape(-1, ee.CHUNK).sum(axis=1)


@pytest.mark.parametrize("name", list(ee.CASES))
def test_census_floors(oracle, name):
    """A condition on the INPUTS, from the oracle's output and the numpy restatement's intermediates alone: the frustum
    culls at least 64 draws and at least 64 are drawn; against the 64 x 64 pyramid the HiZ test removes at least 16 and
    keeps at least 16; and what a case plants is there in the OUTPUT.  The cases too small for a floor carry their reason
    (entity_edges.excused)."""
    c = ee.make_case(name, oracle)
    n, un = c["n"], ee.excused(c)
    assert all(un.values()) and (set(un) <= {"interior_zero_chunk"} or n < 128)
    d0, d2 = {}, {}
    vis0, should0, recs0, _ = _restated(c, 0, n, ee.words(c, "zero"), detail=d0)
    vis2, _, recs2, _ = _restated(c, 2, n, ee.words(c, "zero"), detail=d2)
    if "frustum" not in un:
        assert int((~vis0).sum()) >= 64 and int(should0.sum()) >= 64
    if "occlusion" not in un:
        assert int((d2["reached"] & ~vis2).sum()) >= 16 and int(vis2.sum()) >= 16
    od, _, dropped = _oracle(oracle, c, 0, n, None)
    assert int(od[:4].view(np.uint32)[0]) == min(len(recs0), c["capacity"]) and dropped == max(len(recs0) - c["capacity"], 0)
    per_chunk = _chunk_records(d0["records"], n)
    assert int(per_chunk.sum()) == len(recs0)
    # the rows the restatement evaluated in the last chunk (header N: the active draws), against what the size is for
    rows_last = len(d0["records"][(ee.chunks_of(n) - 1) * ee.CHUNK:])
    assert len(vis0) == len(d2["records"]) == n and rows_last == ee.LAST_CHUNK_DRAWS[n]
    plant, planted = c["plant"], c["planted"]
    if plant == "zero_chunk":
        for k in planted["zero_chunks"]:
            assert per_chunk[k] == 0 and d0["records"][(k + 1) * ee.CHUNK] > 0 and per_chunk[k + 1] > 0
            assert k == 0 or (d0["records"][k * ee.CHUNK - 1] > 0 and per_chunk[k - 1] > 0)
        assert 0 in planted["zero_chunks"] and (len(planted["zero_chunks"]) == 2) == ("interior_zero_chunk" not in un)
    if plant == "fat_chunk":
        many, one = per_chunk[planted["fat_many"]], per_chunk[planted["fat_one"]]
        assert many > ee.EXPAND_TRIP and one > ee.EXPAND_TRIP and (many % 4 or one % 4)
        assert d0["records"][planted["fat_one"] * ee.CHUNK] > ee.EXPAND_TRIP  # ONE owner spans the second trip
        assert d0["records"][planted["fat_many"] * ee.CHUNK:(planted["fat_many"] + 1) * ee.CHUNK].max() < ee.EXPAND_TRIP
    if plant == "ragged":
        at = slice(ee.RAGGED_AT, ee.RAGGED_AT + len(ee.RAGGED))
        assert tuple(d0["meshlets"][at]) == ee.RAGGED and tuple(d2["meshlets"][at]) == ee.RAGGED
    if plant in ee.CLAMPED:
        g = planted["clamped_draw"]
        assert d0["records"][g] == ee.CLAMP_MESHLETS // 32 > c["capacity"] == ee.CLAMP_CAPACITY
        assert per_chunk[g // ee.CHUNK] > c["capacity"] + 1  # what the chunk publishes is cut to capacity + 1
        assert g // ee.CHUNK == dict(clamped_first=0, clamped_middle=n // 2 // ee.CHUNK, clamped_last=ee.chunks_of(n) - 1)[plant]
    if plant == "lod_far":
        assert int((d0["mesh_lod"][should0] >= 1).sum()) >= max(32, int(should0.sum()) // 2)
    elif n >= 128:  # every other case picks LODs on both sides
        assert int((d0["mesh_lod"][should0] >= 1).sum()) >= 32 and int((d0["mesh_lod"][should0] == 0).sum()) >= 1


def _same(got, want_recs, want_words, capacity):
    buf, words, dropped = got
    hdr, recs = L.dispatch_buffer_records(buf)
    assert list(hdr) == [min(len(want_recs), capacity), 1, 1] and dropped == max(len(want_recs) - capacity, 0)
    assert np.array_equal(recs.view(np.uint32), want_recs[:capacity].view(np.uint32)), "records differ"
    if want_words is not None:
        assert np.array_equal(words, want_words), "visibility words differ"


@pytest.mark.parametrize("name", list(ee.CASES))
def test_oracle_equals_numpy_restatement(oracle, name):
    """Two restatements by different means agree bit for bit — records, header and bitset — in passes 0, 1 and 2, with
    the draw buffer's header saying N, N - 300 and N + 300 (the whole-buffer call then processes up to
    ceil(N / 256) x 256 draws), in the contracted profile, and at dispatch sizes 64 and 128 in pass 0."""
    c = ee.make_case(name, oracle)
    cap = c["capacity"]
    for header in ee.header_counts(c["n"]):
        for op, how in ((0, "zero"), (1, "random"), (2, "random"), (2, "ones")):
            vis = ee.words(c, how, seed=op)
            for profile in ((0, 1) if header == c["n"] else (0,)):
                _, _, recs, words = _restated(c, op, header, vis, profile=profile)
                with oracle.arith_profile(profile):
                    _same(_oracle(oracle, c, op, header, vis), recs, words, cap)
        for S in (64, 128):
            _, _, recs, _ = _restated(c, 0, header, None, S=S)
            with oracle.dispatch_size(S):
                _same(_oracle(oracle, c, 0, header, None), recs, None, cap)
    assert oracle.lib().oracle_get_arith_profile() == 0


@pytest.mark.parametrize("name", [k for k in ee.WHOLE if ee.CASES[k]["n"] in ee.RANGE_SIZES])
def test_range_algebra_of_the_oracle(oracle, name):
    """Pass 0: the records of the three shards of ranges(N), concatenated, are the whole call's.  Pass 2: a range call
    leaves every visibility word outside [first / 32, ceil(end / 32)) untouched, and inside writes the whole call's bits
    with zeros past `end`.  The draw buffer claims N + 300 draws throughout: a range is exactly [first, first + n)."""
    c = ee.make_case(name, oracle)
    n, header = c["n"], c["n"] + ee.SLACK
    whole, _, _ = _oracle(oracle, c, 0, n, None)
    shards = ee.dist.shard_ranges(n, 3)
    assert all(r in ee.ranges(n) for r in shards if r[0] < r[1])
    parts = [L.dispatch_buffer_records(_oracle(oracle, c, 0, header, None, first=b, count=e - b)[0])[1] for b, e in shards]
    assert np.array_equal(np.concatenate(parts).view(np.uint32), L.dispatch_buffer_records(whole)[1].view(np.uint32))
    vis = ee.words(c, "random", seed=7)
    _, full, _ = _oracle(oracle, c, 2, n, vis)
    for b, e in ee.ranges(n):
        _, got, _ = _oracle(oracle, c, 2, header, vis, first=b, count=e - b)
        w0, w1 = b // 32, (e + 31) // 32
        assert np.array_equal(got[:w0], vis[:w0]) and np.array_equal(got[w1:], vis[w1:]), (b, e)
        want = full[w0:w1].copy()
        if e % 32:
            want[-1] &= np.uint32((1 << (e % 32)) - 1)
        assert np.array_equal(got[w0:w1], want), (b, e)
    tail = (32 * (n // 32), n)
    assert n % 32 == 0 or (tail in ee.ranges(n) and tail[1] - tail[0] < 32)


def test_the_case_sizes():
    """The sizes are the thresholds of the table, one draw short of them and one past them."""
    assert ee.SIZES == [1, 31, 32, 33, 255, 256, 257, 16383, 16384, 16385, 32513, 32768, 32769, 65536, 65537]
    assert ee.chunks_of(32513) == 128 and 32513 % 256 == 1
    assert ee.header_counts(32768) == [32468, 32768, 33068] and ee.header_counts(1) == [0, 1, 301]
    assert ee.ranges(257) == [(0, 257), (32, 225), (256, 257), (96, 257), (0, 96), (96, 192), (192, 257)]
    assert (96, 96 + 32769) in ee.ranges(65537) and (96, 32769) in ee.ranges(32769)


@pytest.mark.parametrize("constant,source,value", [
    ("kEntityOneLaunchChunks", "entity_cull.hip", ee.ONE_LAUNCH_CHUNKS),
    ("kFusedMaxEntityDraws", "kernels.h", ee.FUSED_MAX),
    ("kShardMaxChunks", "kernels.h", ee.SHARD_MAX_CHUNKS),
    ("kEntityBlock", "entity_common.h", ee.CHUNK),
])
def test_the_table_is_the_codes(constant, source, value):
    """The thresholds the case sizes are derived from, read out of the source text: whoever retunes one moves the cases
    with it."""
    with open(os.path.join(CSRC, source)) as f:
        found = re.findall(r"constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)u?\s*;" % constant, f.read())
    assert found == [str(value)], (constant, found)
    assert ee.EXPAND_TRIP == 4 * ee.CHUNK  # entity_expand_records: U = 4 records per thread and trip
