"""The inputs of the error-map tests (tests/test_error_cpu.py checks what they promise from ``error_ref`` alone, tests/test_error_gpu.py runs
the kernels on them).  A case: a frame, its uint16 ground truth with ~5 % random returns plus hand-placed ones (crop corners, both sides of
every rectangle border, an isolated return, two adjacent returns with different errors, returns on both sides of every row a tile seam can
fall on, raw 0 / at min_depth / at max_depth), and a prediction whose errors span all ten bands and include NaN, +inf, 0 and a negative
value.  Expected pictures come from ``error_ref`` once per (case, radius, background) and are shared, never modified."""
import functools

import numpy as np

import error_ref as ER

TAU = 0.05
SEAM_ROWS = (8, 16, 32, 64)              # a tile of 8, 16, 32 or 64 rows has a seam here (if the crop is that tall)
SEAM_COLS = (64, 128, 256)               # and a tile of 64, 128 or 256 columns here


def _put(case, r, c, raw, pred=None, rel=None):
    """A return at crop (r, c): raw value, and a prediction (given, or gt * (1 + rel))."""
    H, W, top, left, Hc, Wc = case['geom']
    if not (0 <= r < Hc and 0 <= c < Wc):
        return
    case['raw'][top + r, left + c] = raw
    gt = np.float32(raw) / np.float32(case['limits'][0])
    case['pred'][r, c] = np.float32(pred) if pred is not None else np.float32(gt * np.float32(1.0 + rel))
    case['placed'].append((r, c))


def _clear(case, r0, r1, c0, c1):
    H, W, top, left, Hc, Wc = case['geom']
    case['raw'][top + max(r0, 0):top + min(r1, Hc), left + max(c0, 0):left + min(c1, Wc)] = 0


def make_case(geom, rect, seed, limits=ER.LIMITS):
    H, W, top, left, Hc, Wc = geom
    rng = np.random.default_rng(seed)
    hit = rng.random((H, W)) < 0.05
    raw = np.where(hit, rng.integers(300, 20000, (H, W)), 0).astype(np.uint16)
    gt = raw[top:top + Hc, left:left + Wc].astype(np.float32) / np.float32(limits[0])
    rel = np.float32(TAU) * np.exp2(rng.uniform(-6.0, 6.0, (Hc, Wc))).astype(np.float32) * rng.choice([-1.0, 1.0], (Hc, Wc)).astype(np.float32)
    pred = np.where(gt > 0, gt * (1 + rel), rng.uniform(1.0, 80.0, (Hc, Wc))).astype(np.float32)
    case = dict(geom=geom, rect=rect, limits=limits, raw=raw, pred=pred, placed=[],
                frame=rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    r0, r1, c0, c1 = rect
    rm, cm = (r0 + r1) // 2, (c0 + c1) // 2
    _clear(case, rm - 3, rm + 4, cm - 11, cm - 4)                                          # room around the isolated return
    _clear(case, rm - 3, rm + 4, cm + 9, cm + 17)                                          # and around the two neighbours
    for r, c in ((0, 0), (0, Wc - 1), (Hc - 1, 0), (Hc - 1, Wc - 1)):                     # the crop's corners
        _put(case, r, c, 2560, rel=0.3)
    for r, c in ((r0 - 1, cm), (r0, cm + 2), (r1 - 1, cm + 4), (r1, cm + 6), (rm, c0 - 1), (rm + 2, c0), (rm + 4, c1 - 1), (rm + 6, c1)):
        _put(case, r, c, 5120, rel=1.0)                                                    # both sides of the four borders, band 9 if counted
    for j in range(10):                                                                    # one return per band: n = 1.4 * 2^(j - 5)
        _put(case, r0 + 2, c0 + 1 + 3 * j, 4096, rel=TAU * 1.4 * 2.0 ** (j - 5))
    _put(case, rm, cm - 8, 4096, rel=0.04)                                                 # an isolated return
    _put(case, rm, cm + 12, 4096, rel=0.01)                                                # two neighbours: the larger error must win
    _put(case, rm, cm + 13, 4096, rel=0.5)
    for s in SEAM_ROWS:                                                                    # on both sides of every possible seam
        _put(case, s - 1, cm - 16, 3000, rel=0.2)
        _put(case, s, cm - 15, 3000, rel=0.003)
    for s in SEAM_COLS:
        _put(case, rm - 6, s - 1, 3000, rel=0.1)
        _put(case, rm - 5, s, 3000, rel=0.006)
    lo_raw = int(round(limits[1] * limits[0]))                                             # gt == min_depth when that is a multiple of 1 / scale
    for k, v in enumerate((0, lo_raw, lo_raw + 1, int(limits[2] * limits[0]), int(limits[2] * limits[0]) - 1, 65535)):
        _put(case, r0 + 1, c0 + 2 + 2 * k, v, pred=10.0)                                   # raw 0, at / just above min_depth, at / just below max_depth
    for k, p in enumerate((np.nan, np.inf, 0.0, -3.0, -np.inf)):                           # predictions a model should never give
        _put(case, r1 - 2, c0 + 2 + 3 * k, 2560, pred=p)
    return case


GARG = (int(0.40810811 * 70), int(0.99189189 * 70), int(0.03594771 * 264), int(0.96405229 * 264))
CASES = {
    'one-tile-odd-left': make_case((23, 50, 6, 7, 17, 36), (2, 15, 3, 33), 1),                       # every load unaligned
    'tiles-and-remainders': make_case((75, 270, 5, 3, 70, 264), (0, 70, 0, 264), 2),                 # the whole crop counts: corners paint
    'tiles-garg-aligned': make_case((74, 272, 4, 4, 70, 264), GARG, 3),                               # left % 4 == 0, W % 4 == 0: vector loads
    'width-35': make_case((40, 41, 2, 5, 37, 35), (1, 36, 2, 34), 4, limits=(256.0, 1.0 / 256, 80.0)),   # single-frame only: byte stores
}
BATCHABLE = [n for n, c in CASES.items() if c['geom'][5] % 4 == 0]


@functools.lru_cache(maxsize=None)
def expected(name, radius, background, tau=TAU):
    """``(picture, err)`` of ``error_ref.error_image`` for case ``name``: computed once, read-only."""
    c = CASES[name]
    out, err = ER.error_image(c['raw'], c['pred'], c['frame'], c['geom'], c['rect'], tau, radius, background, c['limits'])
    out.setflags(write=False)
    err.setflags(write=False)
    return out, err


# The band rule on every threshold: tau = 1/16 and gt = 16 m (raw 4096) make pred = 16 * (1 +- T[j] * tau) exact in float32, so n == T[j].
THRESHOLD_TAU = 0.0625


def threshold_case():
    """One row: for each of the nine thresholds T[j] a pixel with n == T[j] from below and from above the ground truth, and their
    neighbours one float32 step of the prediction closer to the ground truth (n just under T[j])."""
    preds = []
    for t in ER.T:
        for sign in (-1.0, 1.0):
            p = np.float32(16.0) * np.float32(1.0 + sign * t * THRESHOLD_TAU)
            preds += [p, np.nextafter(p, np.float32(16.0))]
    Wc = len(preds)
    raw = np.full((1, Wc), 4096, np.uint16)
    return dict(geom=(1, Wc, 0, 0, 1, Wc), rect=(0, 1, 0, Wc), limits=ER.LIMITS, raw=raw, pred=np.array([preds], np.float32),
                frame=np.zeros((1, Wc, 3), np.uint8))
