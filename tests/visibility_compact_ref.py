"""numpy restatement of orbit_visibility_compact (include/orbit_abi_ext.h C1-C6), independent of the host mirror: where
the mirror walks the pixels and then the commands, this one COUNTS AND SORTS — the covered words' (command, triangle)
keys are sorted and made unique, the masks are the unique keys scattered into a bit matrix, popcounts are row sums, the
numbering is a cumulative sum over the kept rows, and a region's corner bytes are one gather by the sorted triangle
indices.  It is what tests/test_visibility_compact_cpu.py holds the mirror to; the GPU tests' reference is the mirror."""
import numpy as np

E_CAPACITY, E_RANGE = -3, -9
STAT_NAMES = ("covered_pixels", "foreign_pixels", "visible_commands", "visible_triangles", "written_commands",
              "dropped_commands", "data_words_needed", "range_errors")


def triangle_bits(visibility, n, command_base):
    """C1 -> (bits: bool [n, 256], covered, foreign)"""
    words = np.asarray(visibility, np.uint64).reshape(-1)
    keys = (words[words != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)  # command << 8 | triangle
    k = (keys >> 8) - int(command_base)
    own = (k >= 0) & (k < n)
    pairs = np.unique(k[own] * 256 + (keys[own] & 255))
    bits = np.zeros((n, 256), bool)
    bits[pairs >> 8, pairs & 255] = True
    return bits, len(keys), int((~own).sum())


def pack_masks(bits, max_commands):
    masks = np.zeros(8 * max_commands, np.uint32)
    if len(bits):
        masks[:8 * len(bits)] = np.packbits(bits, axis=1, bitorder="little").reshape(-1).view("<u4")
    return masks


def compact(visibility, draw_commands, max_commands, command_base=0, meshlet_data=None, triangles=False,
            visible_capacity=None, visible_data_words=None, meshlet_data_words=None, fill=0, want_ids=True):
    """The arguments and the result of orbit_amd.raster.host_visibility_compact."""
    words = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)[:4 + 28 * int(max_commands)].view("<u4")
    n = min(int(words[0]), int(max_commands))
    data = None if meshlet_data is None else np.ascontiguousarray(meshlet_data, dtype=np.uint32).reshape(-1)
    data_words = (0 if data is None else len(data)) if meshlet_data_words is None else int(meshlet_data_words)
    cap = int(max_commands) if visible_capacity is None else int(visible_capacity)
    out_words = (len(data) if triangles else 0) if visible_data_words is None else int(visible_data_words)
    bits, covered, foreign = triangle_bits(visibility, n, command_base)
    cmds = words[1:1 + 7 * n].reshape(n, 7).astype(np.int64)
    m = bits.sum(axis=1)
    visible = m > 0
    nt, first_index, index_base = cmds[:, 0] // 3, cmds[:, 2], cmds[:, 3]
    highest = np.where(visible, 255 - np.argmax(bits[:, ::-1], axis=1), -1)  # the largest set t
    consistent = (nt <= 256) & (highest < nt)
    first_word = first_index // 4
    vcount = first_word - index_base
    if triangles:
        consistent &= (first_word >= index_base) & (vcount <= 255) & (first_word <= data_words) \
            & ((first_index + 3 * nt + 3) // 4 <= data_words)
    keep = visible & consistent
    ks = np.flatnonzero(keep)  # ascending k: j is the position in it
    size = (vcount[ks] + (3 * m[ks] + 3) // 4) if triangles else np.zeros(len(ks), np.int64)
    end = np.cumsum(size)
    base = end - size
    written = np.arange(len(ks)) < cap
    if triangles:
        written &= end <= out_words
    nw = int(written.sum())
    assert written[:nw].all()  # C3: a prefix
    new = lambda count: np.full(max(int(count), 1), fill, np.uint32)  # noqa: E731
    out, ids, vdata = new(1 + 7 * cap), new(cap) if want_ids else None, new(out_words) if triangles else None
    rows = cmds[ks[:nw]].copy()
    if triangles:
        rows[:, 0], rows[:, 3], rows[:, 2] = 3 * m[ks[:nw]], base[:nw], 4 * (base[:nw] + vcount[ks[:nw]])
        data_bytes = data.view(np.uint8)
        for k, b in zip(ks[:nw], base[:nw]):
            ts = np.flatnonzero(bits[k])
            corners = np.zeros((3 * len(ts) + 3) // 4 * 4, np.uint8)
            corners[:3 * len(ts)] = data_bytes[(first_index[k] + 3 * ts)[:, None] + np.arange(3)].reshape(-1)
            region = np.concatenate([data[index_base[k]:index_base[k] + vcount[k]], corners.view("<u4")])
            vdata[b:b + len(region)] = region
    out[0] = nw
    out[1:1 + 7 * nw] = rows.astype(np.uint32).reshape(-1)
    if ids is not None:
        ids[:nw] = int(command_base) + ks[:nw]
    errors = int((visible & ~consistent).sum())
    stats = dict(covered_pixels=covered, foreign_pixels=foreign, visible_commands=len(ks), visible_triangles=int(m[ks].sum()),
                 written_commands=nw, dropped_commands=len(ks) - nw, data_words_needed=min(int(size.sum()), 0xFFFFFFFF),
                 range_errors=errors)
    status = E_RANGE if errors else E_CAPACITY if nw < len(ks) else 0
    return dict(masks=pack_masks(bits, int(max_commands)), commands=out[:1 + 7 * cap], ids=None if ids is None else ids[:cap],
                data=None if vdata is None else vdata[:out_words], stats=stats, status=status)


def ranks(masks, k, t):
    """C6 (c): the rank of bit t among the set bits of command k's mask, elementwise."""
    bits = np.unpackbits(np.asarray(masks, "<u4").view(np.uint8).reshape(-1, 32), axis=1, bitorder="little")
    before = np.cumsum(bits, axis=1) - bits
    return before[k, t]
