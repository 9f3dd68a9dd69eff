"""CPU: the premises of the image-ingest tests (tests/ingest_cases.py) and the host side of the feature -- include/mvlt_hip_ingest.h and mvlt_amd/_lib.py
INGEST_PROTOTYPES agree and the older tables are as they were; the reference's identity is the ToTensor table; the integer sums fit; the flip thresholds; the
reference against Pillow; plausible wrong kernels fail the bars; the entry points refuse bad arguments without a device; `content_rect`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ingest_cases as IC
from tests.test_host_cpu import _header_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INGEST = ("mvlt_ingest_version", "mvlt_image_ingest", "mvlt_image_ingest_resize", "mvlt_flip_flags")
CASES = IC.cases()


def _header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_ingest.h")).read()


def test_ingest_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_loss_cpu.py applies to mvlt_hip_loss.h and LOSS_PROTOTYPES)"""
    import mvlt_amd._lib as L
    protos, structs = _header_abi(_header())
    assert set(protos) == set(L.INGEST_PROTOTYPES) == set(INGEST) and not structs
    older = (set(L.PROTOTYPES) | set(L.EXT_PROTOTYPES) | set(L.EMA_PROTOTYPES) | set(L.PLAN_PROTOTYPES) | set(L.OPT_PROTOTYPES) | set(L.LAMB_PROTOTYPES)
             | set(L.LOSS_PROTOTYPES))
    assert not set(INGEST) & older                                # an addition, not an override
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "uint64_t": C.c_uint64}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.INGEST_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    assert protos["mvlt_image_ingest"][1] == ["const uint8_t*", "int", "const float*", "float*", "float*", "const uint8_t*", "int", "int", "int", "int", "float", "void*"]
    assert protos["mvlt_image_ingest_resize"][1] == ["const uint8_t*", "int", "int", "const int*", "const int*", "const uint8_t*", "const float*", "float*", "float*",
                                                    "const uint8_t*", "int", "int", "int", "int", "float", "void*"]
    assert protos["mvlt_flip_flags"][1] == ["uint8_t*", "int", "float", "uint64_t", "uint64_t", "void*"]


def test_ingest_version_sources_and_the_older_tables():
    import mvlt_amd._lib as L
    from mvlt_amd import build, ops
    hdr = _header()
    assert L.lib.mvlt_ingest_version() == L.INGEST_VERSION == int(re.search(r"#define MVLT_INGEST_VERSION (\d+)", hdr).group(1)) == 1
    assert int(re.search(r"#define MVLT_INGEST_MAX_FACTOR (\d+)", hdr).group(1)) == IC.MAX_FACTOR
    assert L.ABI_VERSION == 8 == L.lib.mvlt_abi_version() and L.EXT_VERSION == 1 and L.EMA_VERSION == 1 and L.OPT_VERSION == 1 and L.PLAN_VERSION == 3
    assert L.LAMB_VERSION == 1 and L.LOSS_VERSION == 1 == L.lib.mvlt_loss_version()
    assert len(L.PROTOTYPES) == 61 and len(L.EXT_PROTOTYPES) == 3 and len(L.EMA_PROTOTYPES) == 3 and len(L.PLAN_PROTOTYPES) == 14 and len(L.OPT_PROTOTYPES) == 2
    assert len(L.LAMB_PROTOTYPES) == 5 and len(L.LOSS_PROTOTYPES) == 3
    for name in INGEST:
        assert hasattr(L.lib, name) and name not in L.EXPORTS, name
    assert callable(ops.image_ingest) and callable(ops.image_ingest_resize) and callable(ops.flip_flags)
    src = open(build.__file__).read()
    assert src.count('"mvlt_hip_ingest.h"') == 2                  # source_hash and _deps_mtime
    assert "ingest.hip" in build._sources() and "batchprep.hip" in build._sources()
    kernels = open(os.path.join(ROOT, "mvlt_amd", "csrc", "ingest.hip")).read()
    assert not re.search(r"atomic\w*\s*\(", kernels)
    for k in ("ingest_kernel", "ingest_resize_kernel", "flip_flags_kernel"):
        assert k in kernels, k


def test_reference_identity_is_the_to_tensor_table():
    """at n == m the weights are {0, D, 0} and the reference is v / 255 as ToTensor computes it, bit for bit"""
    w = IC.weights(48, 48, np.arange(48))
    assert np.array_equal(w, np.eye(48, dtype=np.int64) * 96)
    slab = np.zeros((16, 16, 3), dtype=np.uint8)
    slab[..., 0] = np.arange(256).reshape(16, 16)
    slab[..., 1] = np.arange(256)[::-1].reshape(16, 16)
    slab[..., 2] = 7
    got = IC.resample(slab, (0, 0, 16, 16), 16, 16).astype(np.float32)
    table = torch.arange(256).float().div(255).numpy()
    assert np.array_equal(got.view(np.uint32), table[slab.transpose(2, 0, 1)].view(np.uint32))
    from mvlt_amd import ops
    t = ops.ingest_table()
    assert t.shape == (3, 256) and all(np.array_equal(t[c].numpy().view(np.uint32), table.view(np.uint32)) for c in range(3))
    tn = ops.ingest_table(IC.MEAN, IC.STD)
    for c in range(3):
        want = torch.arange(256).float().div(255).sub(torch.tensor(IC.MEAN[c])).div(torch.tensor(IC.STD[c]))      # Normalize: sub_(mean).div_(std) in fp32
        assert torch.equal(tn[c], want)
    assert torch.equal(ops.ingest_norm(IC.MEAN, IC.STD), torch.tensor(IC.MEAN + IC.STD, dtype=torch.float32))


def test_integer_sums_fit_int32_at_the_maximum_factor():
    """2048-pixel side at factor 8: every weighted sum of pixels stays below 2^24 (exact in fp32 too), the weight sums and the tap expression inside int32"""
    n, m = 2048, 256
    w = IC.weights(n, m, np.arange(n))
    assert (w > 0).sum(1).max() <= 2 * IC.MAX_FACTOR + 1
    assert int(w.sum(1).max()) * 255 < 2 ** 24 < 2 ** 31
    assert (2 * n + 1) * m + (2 * m + 1) * n + 2 * n < 2 ** 31
    # the largest side the entry point accepts, at the largest factor: still int32
    n, m = 16384, 2048
    assert 2 * n * (2 * IC.MAX_FACTOR + 1) * 255 < 2 ** 31 and (2 * n + 1) * m + (2 * m + 1) * n + 2 * n < 2 ** 31
    # an upscale never has more than two taps, the rows under a band of 8 output rows / the pixels under a tile of 32 columns stay inside the kernel's LDS arrays
    assert (IC.weights(20, 32, np.arange(20)) > 0).sum(1).max() <= 2
    for n, m in ((256, 32), (384, 48), (77, 32), (255, 32), (20, 32), (1, 32), (2048, 256), (33, 32)):
        pos = IC.weights(n, m, np.arange(n)) > 0
        first, last = pos.argmax(1), n - 1 - pos[:, ::-1].argmax(1)
        for t, room in ((8, 9 * IC.MAX_FACTOR + 1), (32, 33 * IC.MAX_FACTOR + 1)):
            for i0 in range(0, m, t):
                assert last[min(i0 + t, m) - 1] - first[i0] + 1 <= room, (n, m, t, i0)


def test_flip_thresholds():
    assert IC.flip_threshold(0.0) == 0 and IC.flip_threshold(0.5) == 2 ** 23 and IC.flip_threshold(1.0) == 2 ** 24
    assert not IC.flip_flags(5, 100, 64, 0.0).any() and IC.flip_flags(5, 100, 64, 1.0).all()          # a 24-bit draw is never below 0 and always below 2^24
    half = IC.flip_flags(5, 100, 4096, 0.5)
    assert abs(float(half.mean()) - 0.5) < 0.04
    assert np.array_equal(half[7:19], IC.flip_flags(5, 107, 12, 0.5))                                  # counted by sample id, not by position in the batch
    assert IC.STREAM_FLIP not in (IC.BP.STREAM_GRID, IC.BP.STREAM_ROW, IC.BP.STREAM_TOKEN, IC.BP.STREAM_DROPOUT, IC.BP.STREAM_DROPPATH)


def test_reference_is_within_one_level_of_pillow():
    """Pillow rounds the horizontal pass and the result to uint8 (two roundings of convex combinations: at most half a level each) and keeps its coefficients in
    22-bit fixed point (0.01 of a level): the bound is derived, not tuned"""
    Image = pytest.importorskip("PIL.Image")
    worst = 0.0
    for case in CASES:
        for b in range(case.B):
            y0, x0, h, w = (int(v) for v in case.rects[b])
            pil = np.asarray(Image.fromarray(case.src[b, y0:y0 + h, x0:x0 + w]).resize((case.W, case.H), Image.BILINEAR)).astype(np.float64)
            ref = IC.resample(case.src[b], case.rects[b], case.H, case.W).transpose(1, 2, 0) * 255.0
            worst = max(worst, float(np.abs(ref - pil).max()))
            assert np.abs(ref - pil).max() <= 1.01, (case, b, np.abs(ref - pil).max())
    print("largest distance from Pillow, in uint8 levels:", worst)


def test_plausible_wrong_kernels_exceed_the_bar():
    """each of them on at least one case, and by a wide margin"""
    for variant in IC.VARIANTS:
        caught = []
        for case in CASES:
            if variant == "swap_hw" and any(y0 + w > case.src.shape[1] or x0 + h > case.src.shape[2] for y0, x0, h, w in case.rects):
                continue
            err = np.abs(IC.reference(case, variant) - IC.reference(case))
            if (err > 100 * IC.bar(case)).any():
                caught.append(case.name)
        assert caught, variant
        print(variant, "caught by", caught)
    good = [np.abs(IC.reference(c).astype(np.float32).astype(np.float64) - IC.reference(c)).max() / IC.bar(c).min() for c in CASES]
    assert max(good) < 1.0                                        # the reference rounded to fp32 is itself inside every bar


def test_cases_cover_what_they_claim():
    by = {c.name: c for c in CASES}
    assert all(3 <= c.B <= 4 for c in CASES)
    assert all((c.H, c.W) == (32, 48) for c in CASES if c.name != "odd_30x46")
    mf = by["max_factor_8"]
    assert all(h == IC.MAX_FACTOR * mf.H and w == IC.MAX_FACTOR * mf.W for _, _, h, w in mf.rects) and mf.src.shape[1] > 256 and mf.rects[0][0] > 0
    assert IC.taps_v(mf) == 2 * IC.MAX_FACTOR and IC.taps_v(by["identity"]) == 1 and IC.taps_v(by["up_20x31"]) == 2
    one = IC.reference(by["rect_1x1"])
    assert (one == one[:, :, :1, :1]).all()                       # a 1 x 1 rectangle: a constant image
    assert list(by["flip_one_sample"].flip) == [0, 1, 0]
    assert any(c.norm for c in CASES) and any(not c.norm for c in CASES) and any(c.flags is None for c in CASES)
    for c in CASES:
        inside = np.zeros(c.src.shape[:3], dtype=bool)
        for b, (y0, x0, h, w) in enumerate(c.rects):
            inside[b, y0:y0 + h, x0:x0 + w] = True
        assert (c.src[~inside] == 255).all() and c.src[inside].max() <= 100
        assert max(IC.resample(c.src[b], c.rects[b], c.H, c.W).max() for b in range(c.B)) <= 100 / 255 + 1e-12          # no sentinel in any output
        if c.flags is not None:
            assert c.flags.shape == (c.B, 2, 3) and c.flags[0, 0, 0] != c.flags[0, 0, 1] != c.flags[0, 0, 2]


def test_entry_points_refuse_bad_arguments_without_a_device():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    a = 4096                                                     # any non-null, aligned address: the checks never dereference
    bad = lambda good, i, v: good[:i] + [v] + good[i + 1:]
    # src, layout, table, image, masked, flags, B, H, W, patch, fill, stream
    good = [a, 0, a, a, a, a, 2, 32, 48, 16, 1e-6, None]
    f = lib.mvlt_image_ingest
    for i in (0, 2):
        assert f(*bad(good, i, None)) < 0 and b"must not be null" in err(), i
    assert f(*bad(good, 3, None)) < 0 and b"image must not be null" in err()
    assert f(*bad(good, 4, None)) < 0 and b"masked and flags go together" in err()
    assert f(*bad(good, 5, None)) < 0 and b"masked and flags go together" in err()
    assert f(*bad(good, 1, 2)) < 0 and b"layout must be 0" in err()
    assert f(*bad(good, 7, 40)) < 0 and b"multiples of patch" in err()
    assert f(*bad(good, 8, 50)) < 0 and b"multiples of patch" in err()
    assert f(*bad(good, 9, 0)) < 0 and b"multiples of patch" in err()
    assert f(*bad(good, 7, 0)) < 0 and f(*bad(good, 6, -1)) < 0
    assert f(*bad(good, 7, 16384 + 16)) < 0 and b"exceed 16384" in err()
    assert f(*bad(good, 3, a + 2)) < 0 and b"aligned" in err()
    assert f(*bad(good, 6, 0)) == 0                               # nothing to do: no launch
    # src, Hmax, Wmax, rects, rects_host, flip, norm, image, masked, flags, B, H, W, patch, fill, stream
    f = lib.mvlt_image_ingest_resize
    R = lambda *rows: (C.c_int * (4 * len(rows)))(*[v for r in rows for v in r])
    ok = R((0, 0, 64, 64), (10, 20, 54, 44))
    host = lambda r: C.cast(r, C.c_void_p).value
    good = [a, 64, 64, a, host(ok), None, None, a, a, a, 2, 32, 48, 16, 1e-6, None]
    for i in (0, 3, 4):
        assert f(*bad(good, i, None)) < 0 and b"must not be null" in err(), i
    assert f(*bad(good, 8, None)) < 0 and b"masked and flags go together" in err()
    assert f(*bad(good, 11, 40)) < 0 and b"multiples of patch" in err()
    assert f(*bad(good, 1, 0)) < 0 and b"the slab must be" in err()
    assert f(*bad(good, 2, 16385)) < 0 and b"the slab must be" in err()
    assert f(*bad(good, 10, 65536)) < 0 and b"at most 65535 samples" in err()
    for r in ((0, 0, 65, 64), (1, 0, 64, 64), (0, 21, 64, 44), (-1, 0, 10, 10), (0, 0, 0, 10), (0, 0, 10, 0), (60, 60, 2 ** 31 - 1, 1)):
        rr = R((0, 0, 64, 64), r)
        assert f(*bad(good, 4, host(rr))) < 0 and b"rectangle 1" in err() and b"leaves the 64 x 64 slab" in err(), r
    big = [a, 600, 600, a, None, None, None, a, a, a, 1, 32, 48, 16, 1e-6, None]
    for r, fine in (((0, 0, 256, 384), True), ((0, 0, 257, 384), False), ((0, 0, 256, 385), False)):
        rr = R(r)
        if not fine:
            assert f(*bad(big, 4, host(rr))) < 0 and b"exceeds the maximum downscale factor 8" in err(), r
    # (the accepted rectangle would launch: it is run on the GPU by tests/test_ingest_gpu.py)
    assert f(*bad(good, 10, 0)) == 0
    f = lib.mvlt_flip_flags
    assert f(None, 4, 0.5, 1, 0, None) < 0 and f(a, -1, 0.5, 1, 0, None) < 0
    for p in (-0.1, 1.5, float("nan")):
        assert f(a, 4, p, 1, 0, None) < 0 and b"p must be in [0, 1]" in err(), p
    assert f(a, 0, 0.5, 1, 0, None) == 0


def test_ops_have_no_cpu_path():
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    src = torch.zeros(2, 32, 48, 3, dtype=torch.uint8)
    img, flags = torch.zeros(2, 3, 32, 48), torch.zeros(2, 6, dtype=torch.uint8)
    rects = torch.tensor([[0, 0, 32, 48]] * 2, dtype=torch.int32)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.image_ingest(src, ops.ingest_table(), img, img.clone(), flags)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.image_ingest_resize(src, rects, rects, img, img.clone(), flags)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.flip_flags(torch.zeros(2, dtype=torch.uint8), 0.5, 1, 0)


def test_content_rect_restates_the_reference_crop():
    """the reference's lines (mcloader/fashion_gen.py:416-424), literally, on three synthetic images: the crop it returns is the rectangle `content_rect` names"""
    Image = pytest.importorskip("PIL.Image")
    from mvlt_amd.batchprep import content_rect
    rng = np.random.default_rng(3)
    imgs = []
    a = np.full((60, 80, 3), 255, dtype=np.uint8)                 # a dark block on white
    a[10:41, 20:66] = rng.integers(0, 90, size=(31, 46, 3), dtype=np.uint8)
    imgs.append(a)
    b = np.full((50, 50, 3), 255, dtype=np.uint8)                 # two separate blobs, one touching the border
    b[0:5, 30:50] = 0
    b[40:45, 3:9] = 20
    imgs.append(b)
    c = rng.integers(150, 256, size=(40, 70, 3), dtype=np.uint8)  # light grey noise: what is "not white" is decided by convert('1') and its dithering
    c[:6] = 255
    c[:, :9] = 255
    imgs.append(c)
    for arr in imgs:
        img = Image.fromarray(arr)
        img_npy = np.array(img.convert('1'))
        coord = (img_npy == False).nonzero()                      # noqa: E712
        w_top, w_bottom = coord[1].min(), coord[1].max()
        h_top, h_bottom = coord[0].min(), coord[0].max()
        crop_img = img.crop((w_top, h_top, w_bottom, h_bottom)).convert('RGB')
        y0, x0, h, w = content_rect(arr)
        assert crop_img.size == (w, h) and (y0, x0) == (h_top, w_top)
        assert np.array_equal(np.asarray(crop_img), arr[y0:y0 + h, x0:x0 + w])
        assert content_rect(torch.from_numpy(arr)) == (y0, x0, h, w)
    assert content_rect(imgs[0]) == (10, 20, 30, 45)               # the last content row and column are cut, as the reference cuts them
    assert content_rect(np.full((8, 9, 3), 255, dtype=np.uint8)) == (0, 0, 8, 9)
    line = np.full((8, 9, 3), 255, dtype=np.uint8)
    line[4, 2:7] = 0
    assert content_rect(line) == (4, 2, 1, 4)
