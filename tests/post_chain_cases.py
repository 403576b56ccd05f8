"""Inputs for orbit_bloom and orbit_post_process (include/orbit_abi_ext.h B1-B9, T1-T5): hand-built colour planes on the
targets that straddle the kernels' 16 x 16 tiles and the chain's edges.  As in its neighbours, the expected bytes are never
stored: they come from the host mirror or from tests/post_chain_ref.py."""
import numpy as np

F = np.float32

# 1 x 1: one level, no upsample; 1 x 40: one dimension reaches 1 early; 64 x 64: the cap of six levels; 70 x 33: odd halves
# (35, 17, ...); 15 / 16 / 17 and 31 / 32 / 33: one texel either side of one and two tiles of both kernels, as targets and, halved,
# as the levels below; 130 x 70: more than one tile at three levels
TARGETS = ((1, 1), (2, 1), (5, 3), (1, 40), (17, 9), (64, 64), (70, 33), (130, 70), (15, 17), (16, 16), (33, 31), (32, 34))
SMALL_TARGETS = TARGETS[:7]
IMAGES = ("black", "spike", "blaze", "nonfinite", "knee", "checker", "random")
# what each image is run with
SETTINGS = dict(black=dict(), spike=dict(), blaze=dict(), nonfinite=dict(), knee=dict(threshold=1.0, soft_threshold=0.5), checker=dict(),
                random=dict(threshold=0.25, soft_threshold=1.0))


def image(kind, width, height, seed=7):
    """(height, width, 4) float32 HDR colour, alpha 1 as the shade calls leave it"""
    rng = np.random.default_rng(seed + 1000 * width + height)
    c = np.zeros((height, width, 4), F)
    c[..., 3] = 1.0
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "black":
        pass
    elif kind == "spike":  # one texel at 1e6: the Karis average brings it to about 1e3 per group, far below the format's largest value
        c[..., :3] = 0.01
        c[height // 2, width // 2, :3] = (1e6, 3e5, 2e6)
    elif kind == "blaze":  # one texel at 1e12: about 2e6 per group after the Karis average, clamped and counted
        c[..., :3] = 0.01
        c[height // 2, width // 2, :3] = (1e12, 3e11, 2e12)
    elif kind == "nonfinite":  # one NaN and one inf texel (the same one on a 1 x 1 target)
        c[..., :3] = rng.uniform(0.0, 2.0, (height, width, 3))
        c[0, 0, 0] = np.nan
        c[height - 1, width - 1, 1] = np.inf
        c[height // 2, width // 2, 2] = -np.inf
    elif kind == "knee":  # values on both sides of threshold - knee, threshold and threshold + knee
        c[..., :3] = (0.25 + 1.5 * ((xx * 7 + yy * 3) % 11) / 10.0)[..., None] * np.array([1.0, 0.8, 0.6])
    elif kind == "checker":  # every tap straddles texels of different value
        c[..., :3] = np.where(((xx + yy) & 1)[..., None] == 0, np.array([4.0, 0.5, 0.0]), np.array([0.0, 1.5, 8.0]))
    elif kind == "random":  # HDR: mostly dim, a few bright texels, some exact zeros and tiny values
        c[..., :3] = rng.uniform(0.0, 1.0, (height, width, 3)) ** 4 * 3.0
        bright = rng.random((height, width)) < 0.03
        c[bright, :3] *= 200.0
        c[rng.random((height, width)) < 0.05, :3] = 0.0
        c[rng.random((height, width)) < 0.02, :3] = 1e-9
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(c, dtype=F)


def all_cases(targets=TARGETS):
    """[(name, color, bloom settings)]"""
    return [(f"{kind}_{w}x{h}", image(kind, w, h), SETTINGS[kind]) for (w, h) in targets for kind in IMAGES]


# ------------------------------------------------------------------------------- orbit_post_process' trips
# post_process_kernel strides over the pixels from G = min(ceil(pixels / 256), cap) workgroups of 256 threads, the cap being
# num_cus * 8 or what orbit_ctx_set_visibility_grid says: pixel p is lane p % 64 of wave (p % 256) // 64 of workgroup
# (p // 256) % G in that workgroup's trip (p // 256) // G.  The pixel counts either side of a wave, a workgroup and one, two,
# three and four workgroups' worth, as 1 x N planes and a few 2-D ones, under caps of 1, 2 and 3:
POST_THREADS, POST_WAVE = 256, 64
TRIP_COUNTS = (1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 769, 1025)
TRIP_TARGETS = tuple((n, 1) for n in TRIP_COUNTS) + ((33, 31), (65, 9), (16, 33), (257, 3), (64, 5))  # 1023, 585, 528, 771, 320 pixels
TRIP_CAPS = (1, 2, 3)
# where the marked pixels lie: in waves 0, 1 and 3 of the first block of 256, in the three blocks behind it, in the fifth, and
# the plane's last pixel.  A non-finite colour is counted in nonfinite_pixels, a bloom word that is not 0 in bloom_pixels
# (T1: render_mode 0, bloom given and bloom_intensity not 0); no pixel carries both, so the two counters differ
TRIP_NONFINITE = (0, 5, 67, 200, 256, 326, 512, 513, 768, 1024)
TRIP_BLOOM = (1, 63, 65, 130, 255, 257, 300, 511, 514, 700, 769, 1023)
TRIP_BLOOM_WORD = (15 << 6 | 3) | (14 << 6 | 5) << 11 | (16 << 5 | 1) << 22  # B7: about (1.05, 0.54, 2.06), exponent | mantissa per channel


def trip_placement(pixels):
    """-> (nonfinite pixel indices, bloom-marked pixel indices) of a plane of `pixels` pixels: the tables' entries inside
    it and, where there is room, its last pixel (non-finite) and the one before (bloom)"""
    bad = sorted({p for p in TRIP_NONFINITE if p < pixels} | ({pixels - 1} if pixels > 2 else set()))
    lit = sorted({p for p in TRIP_BLOOM if p < pixels and p not in bad} | ({pixels - 2} if pixels > 2 and pixels - 2 not in bad else set()))
    return bad, lit


def trip_image(width, height, marked=True, seed=11):
    """-> (color (height, width, 4) float32, bloom (height * width,) uint32, expect): HDR noise with trip_placement's
    pixels made non-finite (NaN, +inf, -inf in turn, in channel p % 3) and their bloom words set; marked=False leaves
    both out.  expect = dict(pixels, nonfinite_pixels, bloom_pixels) in closed form from the placement"""
    pixels = width * height
    rng = np.random.default_rng(seed + 1000 * width + height)
    c = np.ones((pixels, 4), F)
    c[:, :3] = rng.uniform(0.0, 1.0, (pixels, 3)) ** 3 * 4.0
    bloom = np.zeros(pixels, np.uint32)
    bad, lit = trip_placement(pixels) if marked else ([], [])
    for i, p in enumerate(bad):
        c[p, p % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    bloom[lit] = TRIP_BLOOM_WORD
    return np.ascontiguousarray(c.reshape(height, width, 4)), bloom, dict(pixels=pixels, nonfinite_pixels=len(bad), bloom_pixels=len(lit))


def trip_shape(pixels, cap, resident=2048):
    """What the launch over `pixels` pixels looks like under a cap of `cap` workgroups (0: none) -> dict(grid, trips: per
    workgroup, partial_wave: the last block of 256 ends inside a wave, dead_waves: whole waves of it lie behind the plane)"""
    need = (pixels + POST_THREADS - 1) // POST_THREADS
    grid = min(need, cap if cap else resident, resident)
    trips = [len(range(b, need, grid)) for b in range(grid)]
    tail = pixels - (need - 1) * POST_THREADS  # pixels of the last block, 1..256
    return dict(grid=grid, trips=trips, partial_wave=tail % POST_WAVE != 0, dead_waves=(POST_THREADS - tail) // POST_WAVE)


def trip_shares(marks, pixels, cap, resident=2048):
    """Of the marked pixels `marks`: does a counter fed by them get shares from two trips of one wave, from two waves of
    one workgroup, from two workgroups? -> set of "trips", "waves", "workgroups" """
    grid = trip_shape(pixels, cap, resident)["grid"]
    where = {((p // POST_THREADS) % grid, (p % POST_THREADS) // POST_WAVE, (p // POST_THREADS) // grid) for p in marks}
    out = set()
    if len({(b, w) for b, w, _ in where}) < len(where):
        out.add("trips")
    if any(len({w for b2, w, _ in where if b2 == b}) > 1 for b, _, _ in where):
        out.add("waves")
    if len({b for b, _, _ in where}) > 1:
        out.add("workgroups")
    return out
