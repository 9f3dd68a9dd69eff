"""Test infrastructure: the cases, the exact reference and the bars of the device-side image ingest (csrc/ingest.hip, include/mvlt_hip_ingest.h, docs/ingest.md).

The reference follows the header's definition in exact arithmetic: integer filter weights, integer horizontal sums, the horizontal result rounded to fp32 by
ONE fp32 division (where the kernel rounds), then float64 for the vertical sum, the division by the weight sum, by 255 and the normalisation.  What separates a
kernel from it is the kernel's fp32 rounding of the vertical pass alone: one rounding per tap, one for each of the two divisions, two for (. - mean) / std.
The bar of a case is therefore computed from the case: (taps_v + 4) * 2^-24 on the [0, 1] output, times 1 / std[c] when normalising -- no flat tolerance.

Every slab pixel outside every rectangle is 255 and the inside is dark (<= 100): one stray tap moves an output by a thousand bars.
"""
import numpy as np

from oracle import batchprep_oracle as BP

PATCH, FILL = 16, 1e-6
MAX_FACTOR = 8
STREAM_FLIP = 6
H_OUT, W_OUT = 32, 48
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

VARIANTS = ("no_antialias", "no_half_pixel", "swap_hw", "round_uint8", "no_clip")       # the plausible wrong kernels of tests/test_ingest_cases_cpu.py


class Case:
    def __init__(self, name, slab, rects, H=H_OUT, W=W_OUT, flip=None, norm=False, flags=True, seed=0):
        """slab (Hmax, Wmax); rects: one (y0, x0, h, w) per sample"""
        self.name, self.H, self.W, self.norm = name, H, W, norm
        self.rects = np.asarray(rects, dtype=np.int32)
        self.B = len(rects)
        rng = np.random.default_rng(1000 + seed)
        self.src = np.full((self.B, slab[0], slab[1], 3), 255, dtype=np.uint8)
        for b, (y0, x0, h, w) in enumerate(rects):
            assert 0 <= y0 and 0 <= x0 and y0 + h <= slab[0] and x0 + w <= slab[1] and h >= 1 and w >= 1
            self.src[b, y0:y0 + h, x0:x0 + w] = rng.integers(0, 101, size=(h, w, 3), dtype=np.uint8)
        self.flip = None if flip is None else np.asarray(flip, dtype=np.uint8)
        gh, gw = H // PATCH, W // PATCH
        self.flags = ((np.add.outer(np.arange(gh), np.arange(gw))[None] + np.arange(self.B)[:, None, None]) % 2).astype(np.uint8) if flags else None   # checkerboard

    @property
    def mean_std(self):
        return (MEAN, STD) if self.norm else (None, None)

    def __repr__(self):
        return self.name


def cases():
    return [
        Case("identity", (32, 48), [(0, 0, 32, 48)] * 3, seed=1),
        Case("identity_norm_flip", (32, 48), [(0, 0, 32, 48)] * 3, flip=[1, 0, 1], norm=True, seed=2),
        Case("down_77x101", (90, 120), [(5, 7, 77, 101), (13, 19, 77, 101), (0, 0, 77, 101)], seed=3),
        Case("down_77x101_norm", (90, 120), [(5, 7, 77, 101), (13, 19, 77, 101), (0, 0, 77, 101), (2, 3, 77, 101)], norm=True, seed=4),
        Case("up_20x31", (40, 50), [(3, 4, 20, 31), (20, 19, 20, 31), (0, 0, 20, 31)], seed=5),
        Case("max_factor_8", (272, 400), [(9, 7, 256, 384), (16, 16, 256, 384), (0, 3, 256, 384)], seed=6),
        Case("rect_1x1", (24, 24), [(5, 9, 1, 1), (0, 0, 1, 1), (23, 23, 1, 1)], seed=7),
        Case("aspect_swapped", (100, 100), [(3, 5, 90, 40), (7, 2, 90, 40), (1, 8, 90, 40)], seed=8),
        Case("flip_one_sample", (70, 90), [(4, 6, 60, 75)] * 3, flip=[0, 1, 0], seed=9),
        Case("mixed_rects_norm_flip", (130, 150), [(1, 2, 33, 47), (10, 20, 100, 31), (0, 0, 130, 150), (64, 75, 17, 60)], flip=[1, 1, 0, 0], norm=True, seed=10),
        Case("no_flags", (60, 70), [(2, 3, 50, 61)] * 3, flags=False, seed=11),
        # H and W that are no multiples of 4 (and of no patch: no flags): the element-by-element stores, flipped and not
        Case("odd_30x46", (50, 70), [(3, 5, 41, 57), (0, 0, 30, 46), (1, 0, 20, 70)], H=30, W=46, flip=[0, 1, 1], flags=False, seed=12),
    ]


def weights(n, m, xs, variant=None):
    """(m, len(xs)) integer weights of the input indices xs (relative to the rectangle) for every output index: max(0, D - |(2x+1) m - (2i+1) n|), D = 2 max(n, m)"""
    i, x = np.arange(m, dtype=np.int64)[:, None], np.asarray(xs, dtype=np.int64)[None, :]
    D = 2 * m if variant == "no_antialias" else 2 * max(n, m)
    d = 2 * x * m - 2 * i * n if variant == "no_half_pixel" else (2 * x + 1) * m - (2 * i + 1) * n
    return np.maximum(0, D - np.abs(d))


def taps_v(case):
    """the largest number of vertical taps of any output row of any sample"""
    return max(int((weights(int(h), case.H, np.arange(h)) > 0).sum(1).max()) for _, _, h, _ in case.rects)


def bar(case):
    """per channel, shape (3, 1, 1)"""
    b = (taps_v(case) + 4) * 2.0 ** -24
    return (np.full(3, b) / (np.asarray(STD) if case.norm else 1.0)).reshape(3, 1, 1)


def resample(slab, rect, H, W, variant=None):
    """one sample: slab (Hmax, Wmax, 3) uint8, rect (y0, x0, h, w) -> float64 (3, H, W) in [0, 1]"""
    y0, x0, h, w = (int(v) for v in rect)
    if variant == "swap_hw":
        h, w = w, h
    ys, xs = np.arange(h), np.arange(w)
    if variant == "no_clip":                                         # taps run on into the slab around the rectangle
        ys, xs = np.arange(-y0, slab.shape[0] - y0), np.arange(-x0, slab.shape[1] - x0)
    wx, wy = weights(w, W, xs, variant), weights(h, H, ys, variant)
    region = slab[y0 + ys[0]:y0 + ys[-1] + 1, x0 + xs[0]:x0 + xs[-1] + 1].astype(np.int64)
    assert region.shape[:2] == (len(ys), len(xs))
    sums = np.einsum("jx,yxc->yjc", wx, region)                      # exact
    assert sums.max() < 2 ** 24 and wx.sum(1).min() > 0 and wy.sum(1).min() > 0
    inter = sums.astype(np.float32) / wx.sum(1).astype(np.float32)[None, :, None]          # ONE fp32 division: where the kernel rounds
    assert inter.dtype == np.float32
    if variant == "round_uint8":
        inter = np.floor(inter + np.float32(0.5))
    out = np.einsum("iy,yjc->ijc", wy.astype(np.float64), inter.astype(np.float64)) / wy.sum(1).astype(np.float64)[:, None, None] / 255.0
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def reference(case, variant=None):
    """float64 (B, 3, H, W): resampled, flipped, normalised"""
    out = np.stack([resample(case.src[b], case.rects[b], case.H, case.W, variant) for b in range(case.B)])
    if case.flip is not None:
        out = np.where(case.flip.astype(bool)[:, None, None, None], out[..., ::-1], out)
    if case.norm:
        out = (out - np.asarray(MEAN, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)) / np.asarray(STD, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    return out


def masked_of(case, image):
    """the grid-masked copy of an image (B, 3, H, W) under the case's flags"""
    m = np.repeat(np.repeat(case.flags.astype(bool), PATCH, axis=1), PATCH, axis=2)
    return np.where(m[:, None], np.float32(FILL), image).astype(image.dtype)


def flip_threshold(p):
    """round(p * 2^24), p as the fp32 the entry point receives"""
    return int(np.rint(np.float64(np.float32(p)) * 2.0 ** 24))


def flip_flags(seed, sample0, B, p):
    d = BP.draws(seed, sample0 + np.arange(B, dtype=np.uint64), 0, STREAM_FLIP)[0] >> np.uint32(8)
    return (d.astype(np.int64) < flip_threshold(p)).astype(np.uint8)
