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
