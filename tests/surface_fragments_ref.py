"""orbit_surface_fragments restated in numpy from the rules F1-F8 of include/orbit_abi_ext.h: every operation on arrays of
one float type, each rounded on its own, in the order the rules write them.  Nothing is shared with
orbit_amd/csrc/fragment_common.h; tests/test_surface_fragments_cpu.py holds the host mirror to this, byte for byte.
`dtype=np.float64` evaluates the same definition in float64 from the same inputs (the accuracy tests' reference): then the
outputs are float64 arrays and nothing else changes."""
import numpy as np

OK, E_RANGE = 0, -9
NONE = 0xFFFFFFFF
OUTPUTS = (("world_pos", 4), ("normal", 3), ("tangent", 4), ("uv", 2), ("uv_grad", 4))
SNORM8_BITS = 0x3C010204


def _gather(rows, base, nbytes, dtype):
    """rows: uint8 flat; base: (P,) byte offsets -> (P, nbytes / itemsize) of dtype"""
    idx = base[:, None].astype(np.int64) + np.arange(nbytes, dtype=np.int64)[None, :]
    return np.ascontiguousarray(rows[idx]).view(dtype)


def fragments(visibility, draw_commands, max_commands, meshlets, surface, vertices, vertex_count, entity_data, command_base=0,
              clear=True, into=None, want=("world_pos", "normal", "tangent", "uv", "uv_grad", "material"), vertex_stride=32,
              position_offset=0, normal_offset=12, uv_offset=16, tangent_offset=24, entity_count=None, meshlet_count=None, fill=0,
              dtype=np.float32):
    T = dtype
    vis = np.ascontiguousarray(visibility, np.uint64)
    h, w = vis.shape
    words = np.ascontiguousarray(draw_commands).view(np.uint8).reshape(-1)
    words = words[:len(words) // 4 * 4].view(np.uint32)
    mlt = np.ascontiguousarray(meshlets).view(np.uint8).reshape(-1)
    rows = np.ascontiguousarray(vertices).view(np.uint8).reshape(-1)
    ent = np.ascontiguousarray(entity_data).view(np.uint8).reshape(-1)
    entity_count = len(ent) // 128 if entity_count is None else int(entity_count)
    meshlet_count = len(mlt) // 32 if meshlet_count is None else int(meshlet_count)
    matrices = ent[:len(ent) // 128 * 128].view(np.float32).reshape(-1, 32)
    bary = np.ascontiguousarray(surface["bary"], np.float32).reshape(h, w, 2)
    grad = None if surface.get("grad") is None else np.ascontiguousarray(surface["grad"], np.float32).reshape(h, w, 4)
    triangle = np.ascontiguousarray(surface["triangle"], np.uint32).reshape(h, w, 4)

    out = {}
    for name, per in OUTPUTS + (("material", 1),):
        kind = np.uint32 if name == "material" else np.float32
        if name not in want:
            out[name] = None
        elif into is not None:
            out[name] = np.array(into[name], dtype=kind).reshape(h, w, per)
        else:
            out[name] = np.full((h, w, per), fill, np.uint32).view(kind)
        if out[name] is not None and clear:  # F8
            out[name][...] = NONE if name == "material" else 0.0
        if out[name] is not None and name != "material" and T is not np.float32:
            out[name] = out[name].astype(T)

    # F1
    n = min(int(words[0]), int(max_commands))
    covered = vis != 0
    k = ((vis >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.int64) - int(command_base)
    own = covered & (k >= 0) & (k < n)
    # F2
    unshaded = own & (triangle[..., 0] == NONE)
    rest = own & ~unshaded
    ys, xs = np.nonzero(rest)
    cmd = words[1:1 + 7 * n].reshape(-1, 7)[k[ys, xs]] if len(ys) else np.zeros((0, 7), np.uint32)
    tri = triangle[ys, xs].astype(np.int64)
    bad = (tri[:, 0] >= entity_count) | (tri[:, 0] != cmd[:, 4]) | (tri[:, 1:] >= int(vertex_count)).any(axis=1) | (cmd[:, 6] >= meshlet_count)
    stale = np.zeros((h, w), bool)
    stale[ys[bad], xs[bad]] = True
    ys, xs, tri, cmd = ys[~bad], xs[~bad], tri[~bad], cmd[~bad]
    P = len(ys)
    stats = dict(covered_pixels=int(covered.sum()), written_pixels=P, foreign_pixels=int((covered & ~own).sum()),
                 unshaded_pixels=int(unshaded.sum()), stale_pixels=int(stale.sum()), degenerate_pixels=0)
    result = dict(out, stats=stats, status=E_RANGE if stats["stale_pixels"] else OK, written=(ys, xs))
    if P == 0:
        return result

    snorm = np.array([SNORM8_BITS], np.uint32).view(np.float32)[0].astype(T)
    m = matrices[tri[:, 0]].astype(T)  # (P, 32): model, normal
    one = T(1.0)

    def direction(v):  # F3: normalize(M3 x v)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        d = [(m[:, 16 + r] * x + m[:, 20 + r] * y) + m[:, 24 + r] * z for r in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return np.stack([d[r] / length for r in range(3)], axis=1)

    corners = []
    with np.errstate(all="ignore"):
        for c in range(3):
            base = tri[:, 1 + c] * int(vertex_stride)
            pos = _gather(rows, base + int(position_offset), 12, np.float32).astype(T)
            n8 = _gather(rows, base + int(normal_offset), 4, np.int8).astype(T) * snorm
            t8 = _gather(rows, base + int(tangent_offset), 4, np.int8).astype(T) * snorm
            uv = _gather(rows, base + int(uv_offset), 8, np.float32).astype(T)
            x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
            wp = np.stack([((m[:, r] * x + m[:, 4 + r] * y) + m[:, 8 + r] * z) + m[:, 12 + r] * one for r in range(4)], axis=1)
            corners.append(dict(world_pos=wp, normal=direction(n8), tangent=np.concatenate([direction(t8), t8[:, 3:4]], axis=1), uv=uv))
        # F4
        l1, l2 = bary[ys, xs, 0].astype(T), bary[ys, xs, 1].astype(T)
        l0 = (one - l1) - l2
        l0 = np.where(l0 < 0, T(0.0), l0)
        vals = {}
        for name, _ in OUTPUTS[:4]:
            a = [c[name] for c in corners]
            vals[name] = (a[0] * l0[:, None] + a[1] * l1[:, None]) + a[2] * l2[:, None]
        # F5
        vals["uv_grad"] = np.zeros((P, 4), T)
        e1, e2 = corners[1]["uv"] - corners[0]["uv"], corners[2]["uv"] - corners[0]["uv"]
        if grad is not None:
            g = grad[ys, xs].astype(T)
            for i in range(2):
                vals["uv_grad"][:, i] = e1[:, i] * g[:, 0] + e2[:, i] * g[:, 1]
                vals["uv_grad"][:, 2 + i] = e1[:, i] * g[:, 2] + e2[:, i] * g[:, 3]
    # F7
    degenerate = np.zeros(P, bool)
    for name, _ in OUTPUTS:
        finite = np.isfinite(vals[name])
        degenerate |= ~finite.all(axis=1)
        vals[name] = np.where(finite, vals[name], T(0.0))
    stats["degenerate_pixels"] = int(degenerate.sum())
    for name, _ in OUTPUTS:
        if out[name] is not None:
            out[name][ys, xs] = vals[name]
    if out["material"] is not None:  # F6
        out["material"][ys, xs, 0] = _gather(mlt, cmd[:, 6].astype(np.int64) * 32 + 28, 2, np.uint16)[:, 0]
    result.update(out)
    result["detail"] = dict(corners=corners, e1=e1, e2=e2, degenerate=degenerate, vals=vals)
    return result
