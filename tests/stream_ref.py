"""A plain NumPy model of a derived meshlet stream (include/orbit_abi_ext.h, "Derived meshlet streams"; the kernels of
orbit_amd/csrc/meshlet_stream.hip): what the header and the comments promise of the arrays, stated meshlet by meshlet
with no word, wave or block arithmetic in it except where a promise is about words (base32, the block bounds).  Nothing
of the product is asked but the host export of a block's bound (`bounds_of`, tests/test_block_pretest_cpu.py).

    ref = StreamRef(first, capacity)          zero-filled arrays, class 3 everywhere, nothing readable
    ref.update(source_id, meshlets, lo, n)    orbit_meshlet_stream_update of the n Meshlets of [lo, lo + n)
    ref.set_materials(table or None)          orbit_meshlet_stream_set_materials (MATERIAL records)
    ref.views()                               what orbit_meshlet_stream_read_arrays and _block_bounds read back

What is compared and what is not: every per-meshlet array byte for byte over the whole capacity; base32 at every
multiple of 32 inside the capacity; the class of every meshlet inside the capacity; the block bound of every block that
holds a meshlet of the capacity; a link bit only where `link_cared` says so — meshlet m and m - 1 both derived from the
current source (the build kernel documents every other link bit as arbitrary: "derived earlier (or never: then the bit is
as arbitrary as the rest)").  Bits of words that belong to meshlets outside the capacity are never compared.
"""
import numpy as np

from orbit_amd import layouts as L
from test_block_pretest_cpu import BOUND, bounds_of


def meshlet_words(meshlets):
    """Meshlet records as u32[n, 8]: words 0..3 the sphere, 4 the cone, 5 vertex_offset, 6 data_offset, 7 material_index |
    vertex_count << 16 | triangle_count << 24."""
    return np.ascontiguousarray(meshlets, dtype=L.MESHLET).view(np.uint32).reshape(-1, 8)


def data_words(vertex_count, triangle_count):
    """meshlet_data_words (kernels.h): the vertex indices, then the triangle bytes rounded up to words."""
    return vertex_count.astype(np.uint32) + ((triangle_count.astype(np.uint32) * 3 + 3) >> 2)


class StreamRef:
    def __init__(self, first, capacity):
        self.first, self.capacity = int(first), int(capacity)
        n = self.capacity
        self.word0 = self.first >> 5
        self.words = ((self.first + n - 1) >> 5) - self.word0 + 1
        self.sphere = np.zeros((n, 4), np.uint32)
        self.cone = np.zeros(n, np.uint32)
        self.mat = np.zeros(n, np.uint16)
        self.cmd = np.zeros((n, 3), np.uint32)
        self.cnt = np.zeros(n, np.uint16)
        self.link = np.zeros(n, bool)
        self.cls = np.full(n, 3, np.uint8)       # all-ones planes: "look the material up"
        self.base32 = np.zeros((self.words, 2), np.uint32)
        self.blk = np.zeros(self.words, BOUND)   # not valid until derived
        self.derived = np.zeros(n, bool)         # from the current source
        self.source = None
        self.lo = self.hi = 0                    # the hull: what a cull may read
        self.materials = None

    # -------------------------------------------------------------------------------------------------- operations
    def _classes(self, mat):
        """The class of material indices `mat`: the material's alpha_mode if it is below 3 and the index is inside the
        table, else 3."""
        if self.materials is None:
            return np.full(len(mat), 3, np.uint8)
        mode = self.materials["alpha_mode"]
        inside = mat < len(mode)
        m = mode[np.where(inside, mat, 0)]
        return np.where(inside & (m < 3), m, 3).astype(np.uint8)

    def set_materials(self, table):
        """Re-derives the class of every meshlet of the capacity from `mat` (zero where nothing was derived)."""
        self.materials = None if table is None else np.ascontiguousarray(table, dtype=L.MATERIAL).copy()
        self.cls = self._classes(self.mat)

    def update(self, source_id, meshlets, lo, n):
        lo, n = int(lo), int(n)
        assert self.first <= lo and lo + n <= self.first + self.capacity
        if n == 0:
            return
        w = meshlet_words(meshlets)
        assert len(w) == n
        a, b = lo - self.first, lo - self.first + n
        # the hull grows with the same source and starts over with another; the arrays keep their values outside [lo, lo + n)
        if source_id == self.source and self.hi > self.lo:
            self.lo, self.hi = min(self.lo, lo), max(self.hi, lo + n)
        else:
            self.source, self.lo, self.hi = source_id, lo, lo + n
            self.derived[:] = False
        self.derived[a:b] = True
        # the re-layout of a Meshlet
        self.sphere[a:b] = w[:, 0:4]
        self.cone[a:b] = w[:, 4]
        self.mat[a:b] = w[:, 7] & 0xFFFF
        self.cmd[a:b] = w[:, 5:8]
        self.cnt[a:b] = w[:, 7] >> 16
        g = np.arange(lo, lo + n)
        at32 = g % 32 == 0
        self.base32[(g[at32] >> 5) - self.word0] = w[at32][:, 5:7]
        self.cls[a:b] = self._classes(self.mat[a:b])
        # the link bit of m in [lo, lo + n], from the stream's own copy (which now holds the range): m continues m - 1's
        # chain; false at the stream's first meshlet
        m = np.arange(max(a, 1), min(b + 1, self.capacity))
        p = self.cmd[m - 1]
        size = data_words((p[:, 2] >> 16) & 0xFF, p[:, 2] >> 24)
        self.link[m] = (self.cmd[m, 0] == p[:, 0]) & (self.cmd[m, 1] == p[:, 1] + size)  # (u32: wraps like the kernel's)
        if a == 0:
            self.link[0] = False
        # the bounds of the blocks the update touched: per block, over those of its meshlets that lie inside the
        # capacity, as the sphere array now stands (never-derived zero spheres included)
        b0, b1 = lo >> 5, ((lo + n - 1) >> 5) + 1
        f0 = max(b0, (self.first + 31) >> 5)                 # the touched blocks that lie wholly inside the capacity:
        f1 = max(min(b1, (self.first + self.capacity) >> 5), f0)  # one call of the export for all of them
        if f1 > f0:
            self.blk[f0 - self.word0:f1 - self.word0] = bounds_of(
                self.sphere[f0 * 32 - self.first:f1 * 32 - self.first].view(np.float32))
        for blk in [x for x in range(b0, b1) if not f0 <= x < f1]:
            i0, i1 = max(blk * 32 - self.first, 0), min(blk * 32 + 32 - self.first, self.capacity)
            self.blk[blk - self.word0] = bounds_of(self.sphere[i0:i1].view(np.float32))[0]

    # -------------------------------------------------------------------------------------------------------- views
    def _pack(self, bits):
        """Per-meshlet booleans -> the words of global index / 32 that hold the capacity (bits outside it clear)."""
        pad = np.zeros(self.words * 32, bool)
        off = self.first - self.word0 * 32
        pad[off:off + self.capacity] = bits
        return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)

    def views(self):
        """-> dict: the arrays as orbit_meshlet_stream_read_arrays over the whole capacity returns them (`link`, `cls0`,
        `cls1` with the bits outside the capacity clear), `blk` as orbit_meshlet_stream_block_bounds does, and the
        masks that say which bits are compared: `inside` (words: meshlets of the capacity), `link_cared` (words),
        `base32_cared` (per entry: the multiple of 32 lies inside the capacity); `hull` = (lo, hi)."""
        both = self.derived.copy()
        both[1:] &= self.derived[:-1]
        both[0] = self.derived[0]  # the stream's first meshlet: its bit is false by definition
        g0 = (np.arange(self.words) + self.word0) * 32
        return dict(sphere=self.sphere.copy(), cone=self.cone.copy(), mat=self.mat.copy(), cmd=self.cmd.copy(),
                    cnt=self.cnt.copy(), link=self._pack(self.link), cls0=self._pack((self.cls & 1) != 0),
                    cls1=self._pack((self.cls & 2) != 0), base32=self.base32.copy(), blk=self.blk.copy(),
                    inside=self._pack(np.ones(self.capacity, bool)), link_cared=self._pack(both),
                    base32_cared=(g0 >= self.first) & (g0 < self.first + self.capacity), hull=(self.lo, self.hi))


def assert_views_equal(got, want, what=""):
    """`got`: read_arrays' dict plus `blk`; `want`: StreamRef.views().  Byte-exact, bits under their masks."""
    for k in ("sphere", "cone", "mat", "cmd", "cnt"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs at {np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1))[:8]}"
    c = want["base32_cared"]
    assert np.array_equal(got["base32"][c], want["base32"][c]), f"{what}: base32 differs at entries {np.flatnonzero((got['base32'] != want['base32']).any(1) & c)[:8]}"
    for k, mask in (("cls0", want["inside"]), ("cls1", want["inside"]), ("link", want["link_cared"])):
        diff = (got[k] ^ want[k]) & mask
        assert not diff.any(), f"{what}: {k} differs in words {np.flatnonzero(diff)[:8]} (bits {[hex(int(x)) for x in diff[diff != 0][:8]]})"
    assert got["blk"].tobytes() == want["blk"].tobytes(), \
        f"{what}: block bounds differ at blocks {np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(got['blk'], want['blk'])])[:8]}"
