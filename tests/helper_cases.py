"""Test infrastructure: inputs and float64 references of the layout and index helper kernels of csrc/elementwise.hip -- weight_prep, transpose_cast,
patchify / patchify_strip, gather_rows / scatter_rows, masked_select / masked_select_loop, row_scale, head_grad_prep, resize_tokens / resize_tokens_multi
(tests/test_helper_edges_gpu.py runs them on the GPU; tests/test_helper_cases_cpu.py pins the premises of the inputs on the CPU).

Plain numpy, on the CPU; the library is not imported.  Everything except a non-dyadic resize is data movement: the reference is a float64 array, the
kernel's result must equal it BIT FOR BIT after one rounding to the output dtype (`as_stored`), and `mismatch` names the first element that does not.
The values tell positions apart: `coded` (row * 1024 + column, exact in fp32) where the output is fp32, `ints` (small integers, exact in bf16) and `fracs`
(the same plus sixteenths: more than 8 significant bits, so that the one rounding of a bf16 output shows) where it is bf16.

The host dispatch conditions of csrc/elementwise.hip are restated next to the cases that depend on them (patchify_route, ms_kernel, prep_search, head_rstep,
row_trips): the CPU file asserts that every case reaches the branch it is there for.
"""
import types

import numpy as np

NS = types.SimpleNamespace
SENTINEL = 7.0
DTYPES = ("bf16", "fp32")
NT = 256                                         # threads per workgroup of every kernel here but the two masked_select ones


# ================================================================================================ rounding and comparison
def bf16_round(a):
    """float64 values that are exact in fp32 -> the nearest bf16, ties to even, as float64"""
    a = np.asarray(a, dtype=np.float64)
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a), "the reference must be exact in fp32 before its one rounding"
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def as_stored(ref, dt):
    """the float64 reference as the kernel must store it: rounded once to bf16, or exactly the fp32 value; -> float32 array (bf16 widened)"""
    ref = np.asarray(ref, dtype=np.float64)
    if dt == "bf16":
        return bf16_round(ref).astype(np.float32)
    f = ref.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), ref), "an fp32 reference must be exact"
    return f


def mismatch(got, want, where=None):
    """bit-for-bit comparison of two float32 (or two integer) arrays, optionally only where `where` is set; None, or a message that names the first
    element that differs"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"shape {got.shape} against {want.shape}"
    if got.dtype == np.float32:
        bad = got.view(np.uint32) != np.asarray(want, dtype=np.float32).view(np.uint32)
    else:
        bad = got != want
    if where is not None:
        bad = bad & where
    if not bad.any():
        return None
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    return f"{int(bad.sum())} of {bad.size} elements differ, first at element {at}: got {got[at]!r}, want {want[at]!r}"


def assert_same(name, got, ref, dt, where=None):
    msg = mismatch(np.asarray(got, dtype=np.float32), as_stored(ref, dt), where)
    assert msg is None, f"{name} ({dt}): {msg}"


# ================================================================================================ values that tell positions apart
def coded(rows, cols, row0=0):
    """row * 1024 + column: unique below 2^24 for rows < 16384, cols <= 1024"""
    assert cols <= 1024 and row0 + rows <= 16384
    return (np.arange(row0, row0 + rows)[:, None] * 1024 + np.arange(cols)[None, :]).astype(np.float64)


def ints(rows, cols, mod=121):
    """(7 row + 13 column) % mod - mod // 2: integers of at most 7 bits (exact in bf16, their pairwise sums too), different for neighbours in either
    direction and for the transposed position"""
    assert mod <= 127
    return ((7 * np.arange(rows)[:, None] + 13 * np.arange(cols)[None, :]) % mod - mod // 2).astype(np.float64)


def fracs(rows, cols):
    """ints plus a position-dependent number of sixteenths: up to 11 significant bits, so a bf16 output is rounded, and rounded once"""
    return ints(rows, cols) + ((3 * np.arange(rows)[:, None] + 5 * np.arange(cols)[None, :]) % 16) / 16.0


def values(rows, cols, dt, rounded=False):
    """operand values for an output of dtype dt; rounded: a bf16 output must show its rounding"""
    if dt == "fp32":
        return coded(rows, cols)
    return fracs(rows, cols) if rounded else ints(rows, cols)


def phys_rows(rows, rmap=None):
    """physical row of every logical row under a mode-0 row map (rows_per_batch, batch_stride, offset); None: the identity"""
    r = np.arange(rows)
    if rmap is None:
        return r
    rpb, stride, off = rmap
    return (r // rpb) * stride + off + r % rpb


# ================================================================================================ weight_prep
TS = 64                                          # tile of kind 0 / 2
PREP_MAXD = 1024                                 # descriptors whose blk_start fits the LDS copy the search runs on
PREP_T0 = ((1, 1), (63, 65), (64, 64), (65, 63), (130, 7))                 # kind 0 (R, C), each with ld_out = R and R + 5
PREP_T2 = ((64, 64, 64), (60, 72, 64), (8, 136, 16), (64, 8, 72))          # kind 2 (R, C, ld_out); the last: ld_out beyond the tile edge


def prep_search(ndesc):
    """where the block -> descriptor search of a launch WITHOUT blk_desc reads blk_start (weight_prep_kernel: in_lds = ndesc <= MAXD)"""
    return "lds" if ndesc <= PREP_MAXD else "global"


def prep_blocks(d):
    return (d.d0 * d.d1 * d.d2 + NT - 1) // NT if d.kind == 1 else ((d.R + TS - 1) // TS) * ((d.C + TS - 1) // TS)


def desc(kind, src, dst, *, R=0, C=0, ld_out=0, dims=(0, 0, 0), src_off=0, ss=(0, 0, 0), ds=(0, 0, 0)):
    """one mvlt_prep_desc; src / dst = (buffer index, element offset) into the case's buffers"""
    return NS(kind=kind, src=src, dst=dst, R=R, C=C, ld_out=ld_out, d0=dims[0], d1=dims[1], d2=dims[2], src_off=src_off,
              ss0=ss[0], ss1=ss[1], ss2=ss[2], ds0=ds[0], ds1=ds[1], ds2=ds[2])


def prep_written_cols(d):
    """columns [0, n) of every row of W^T that a transpose descriptor writes: kind 0 exactly R (the padding [R, ld_out) is left alone); kind 2 whole
    16-byte pieces up to the edge of its last row tile or ld_out, whichever comes first -- zeros from R on (the tile's rows >= R are loaded as zeros)"""
    return d.R if d.kind == 0 else min(d.ld_out, (d.R + TS - 1) // TS * TS)


def prep_ref(case):
    """-> per destination buffer (float64 values, written mask); an element that is not written must keep its sentinel"""
    outs = [(np.zeros(n), np.zeros(n, dtype=bool)) for n in case.dst_sizes]
    for d in case.descs:
        src = case.srcs[d.src[0]][0][d.src[1]:]
        want, wr = outs[d.dst[0]]
        if d.kind in (0, 2):
            n = prep_written_cols(d)
            block = np.zeros((d.C, n))
            block[:, :d.R] = src[:d.R * d.C].reshape(d.R, d.C).T
            at = d.dst[1] + np.arange(d.C)[:, None] * d.ld_out + np.arange(n)[None, :]
        else:
            i0, i1, i2 = np.meshgrid(np.arange(d.d0), np.arange(d.d1), np.arange(d.d2), indexing="ij")
            block = src[d.src_off + i0 * d.ss0 + i1 * d.ss1 + i2 * d.ss2]
            at = d.dst[1] + i0 * d.ds0 + i1 * d.ds1 + i2 * d.ds2
        assert not wr[at].any(), "destinations are distinct"
        want[at], wr[at] = block, True
    return outs


def _prep_case(name, dt, parts):
    """parts: (kind, source values (float64, flat), destination size, keyword arguments of desc) -- one source and one destination buffer each"""
    srcs, sizes, descs = [], [], []
    for k, (kind, src, size, kw) in enumerate(parts):
        srcs.append((np.asarray(src, dtype=np.float64).reshape(-1), "bf16" if kind == 2 else "fp32"))
        sizes.append(size)
        descs.append(desc(kind, (k, 0), (k, 0), **kw))
    return NS(name=name, dt=dt, srcs=srcs, dst_sizes=sizes, descs=descs)


def _transpose_part(kind, R, C, ld_out, dt):
    src = ints(R, C) if kind == 2 else values(R, C, dt, rounded=True)
    return (kind, src, C * ld_out, dict(R=R, C=C, ld_out=ld_out))


def _gather_part(dims, src_off, ss, ds, dt, src_size=None, dst_size=None):
    n = dims[0] * dims[1] * dims[2]
    hi = lambda off, s: off + sum((e - 1) * t for e, t in zip(dims, s) if t > 0)
    src_size = src_size or hi(src_off, ss) + 1
    dst_size = dst_size or hi(0, ds) + 1
    assert n >= 1
    src = values((src_size + 63) // 64, 64, dt, rounded=True).reshape(-1)[:src_size]
    return (1, src, dst_size, dict(dims=dims, src_off=src_off, ss=ss, ds=ds))


def _contig(dims):
    return (dims[1] * dims[2], dims[2], 1)


def prep_gather_parts(dt):
    """name -> part.  n255 / n256 / n257: a 3-D gather whose source is laid out [d2][d1][d0] (every stride in play), one element short of a workgroup, one
    workgroup, one element into a second; n257 writes rows of 8 of which it fills 1 (the gaps keep their sentinel).  flipped: the dgrad taps of a 3x3 conv,
    dst (cin, 8 - t, out) <- src[out][cin][t], a NEGATIVE source stride behind src_off = t - 1.  permute: [out][cin][kh][kw] -> [out][kh][kw][cin]."""
    parts = {}
    for name, dims in (("n255", (3, 5, 17)), ("n256", (4, 8, 8)), ("n257", (257, 1, 1))):
        ss = (1, dims[0], dims[0] * dims[1])
        ds = _contig(dims) if name != "n257" else (8, 1, 0)
        parts[name] = _gather_part(dims, 0, ss, ds, dt)
    cin, t, out = 3, 9, 5
    parts["flipped"] = _gather_part((cin, t, out), t - 1, (t, -1, cin * t), (t * out, out, 1), dt, src_size=out * cin * t)
    out, cin, t = 4, 3, 4
    parts["permute"] = _gather_part((out, t, cin), 0, (cin * t, 1, t), (t * cin, cin, 1), dt)
    return parts


def prep_single_cases(dt):
    """one descriptor per table: every kind 0 / kind 2 shape (kind 2 only for bf16) and every gather"""
    cases = []
    for R, C in PREP_T0:
        for ld in (R, R + 5):
            cases.append(_prep_case(f"kind0-{R}x{C}-ld{ld}", dt, [_transpose_part(0, R, C, ld, dt)]))
    if dt == "bf16":
        for R, C, ld in PREP_T2:
            cases.append(_prep_case(f"kind2-{R}x{C}-ld{ld}", dt, [_transpose_part(2, R, C, ld, dt)]))
    for name, part in prep_gather_parts(dt).items():
        cases.append(_prep_case(f"kind1-{name}", dt, [part]))
    return cases


def prep_mixed_case(dt):
    """every kind in one table, a one-block gather first: the first blocks are 0, 1, 3, 5 (, 7), 8, 11 -- no descriptor but the first starts on a multiple of
    its own tile count, and the search has to tell six (five) descriptors apart"""
    g = prep_gather_parts(dt)
    parts = [g["n255"], _transpose_part(0, 65, 63, 70, dt), g["n257"]]
    if dt == "bf16":
        parts.append(_transpose_part(2, 60, 72, 64, dt))
    parts += [g["flipped"], _transpose_part(0, 130, 7, 130, dt), g["permute"]]
    return _prep_case("mixed", dt, parts)


def prep_many_case(dt, n=PREP_MAXD + 1):
    """n one-block descriptors (kind 1, one element each) out of ONE source into ONE destination: descriptor i copies src[perm[i]] to dst[i]"""
    perm = (np.arange(n) * 397 + 11) % n                         # 397 is prime to 1025: a permutation
    src = values((n + 63) // 64, 64, dt, rounded=True).reshape(-1)[:n]
    descs = [desc(1, (0, int(perm[i])), (0, i), dims=(1, 1, 1)) for i in range(n)]
    return NS(name=f"many{n}", dt=dt, srcs=[(src, "fp32")], dst_sizes=[n], descs=descs)


# ================================================================================================ transpose_cast
TRANSPOSE_SHAPES = ((1, 1), (33, 1))             # (R, C): one element; one row past the first 32-row tile, a single column


def transpose_ref(x):
    return x.T


def transpose_tiled(x, T, *, keep_tile=None, swap_bounds=False):
    """the tiled transpose a kernel runs, and two ways of getting it wrong: keep_tile = (tr, tc): that tile's elements are written to the right tile but
    not transposed inside it; swap_bounds: the ragged-tile bound checks r against C and c against R.  Elements a kernel does not write stay NaN."""
    R, C = x.shape
    out = np.full((C, R), np.nan)
    for tr in range((R + T - 1) // T):
        for tc in range((C + T - 1) // T):
            for j in range(T):
                for i in range(T):
                    r, c = tr * T + j, tc * T + i
                    ok = (r < C and c < R) if swap_bounds else (r < R and c < C)
                    if not ok or r >= R or c >= C:
                        continue
                    if keep_tile == (tr, tc):
                        rr, cc = tr * T + i, tc * T + j                      # the element of the mirrored place inside the tile
                        out[c, r] = x[rr, cc] if rr < R and cc < C else 0.0
                    else:
                        out[c, r] = x[r, c]
    return out


# ================================================================================================ patchify
# (k, Cin, B, H, W, out offset in elements, route)
PATCHIFY_CASES = (
    (2, 8, 2, 6, 10, 0, "generic"),
    (8, 1, 2, 16, 24, 0, "generic"),
    (4, 4, 2, 8, 12, 0, "generic"),
    (4, 3, 2, 8, 16, 1, "generic"),              # the model's shape, `out` one element off its 16-byte boundary
    (4, 3, 1, 4, 1364, 0, "generic"),            # a strip of 12 x (W + 4) floats is past 64 KB of LDS
    (4, 3, 1, 4, 4, 0, "strip"),                 # one strip, one patch
    (4, 3, 1, 8, 1360, 0, "strip"),              # the widest strip that fits: 340 patches, two trips of the store loop of 256 threads
    (4, 3, 3, 12, 20, 0, "strip"),               # several samples and strips: blockIdx -> (b, oi)
)


def patchify_route(k, Cin, W, img_aligned=True, out_aligned=True):
    """mvlt_patchify: the strip kernel takes k = 4, Cin = 3, whole 16-byte groups, a strip that fits 64 KB, and 16-byte aligned pointers"""
    return "strip" if (k == 4 and Cin == 3 and W % 4 == 0 and 12 * (W + 4) * 4 <= 65536 and img_aligned and out_aligned) else "generic"


def patchify_image(B, Cin, H, W, dt):
    n = B * Cin * H * W
    if dt == "fp32":
        assert n < 2 ** 24
        return (np.arange(n) + 0.25).reshape(B, Cin, H, W)
    i = np.arange(n)
    return (((7 * i) % 251 - 125) + ((3 * i) % 16) / 16.0).reshape(B, Cin, H, W)       # up to 11 significant bits


def patchify_ref(img, k):
    """P[(b, oi, oj), (c, di, dj)] = img[b, c, oi k + di, oj k + dj]"""
    B, Cin, H, W = img.shape
    return img.reshape(B, Cin, H // k, k, W // k, k).transpose(0, 2, 4, 1, 3, 5).reshape(B * (H // k) * (W // k), Cin * k * k)


# ================================================================================================ gather / scatter
PIECE = {"bf16": 8, "fp32": 4}                   # elements of one 16-byte piece
ROW_MAP = (5, 9, 2)                              # rows_per_batch, batch_stride, offset: all three non-trivial
# (rows, wide): C = one piece, or 520.  2049 rows of 520: the largest of the issue's cases -- 133185 (bf16) / 266370 (fp32) pieces, ONE trip of the
# grid-stride loop; the second trip needs more than 4096 x 256 pieces: 16140 rows of 520 bf16, 8070 rows of 520 fp32 (17 MB each)
ROWS_CASES = ((1, False), (1, True), (37, False), (2049, True))
ROWS_SECOND_TRIP = {"bf16": 16140, "fp32": 8070}


def row_trips(rows, C, dt):
    """trips of the grid-stride loop of gather_rows_kernel / scatter_rows_kernel: grid_for(rows * C / PC) caps the grid at 4096 workgroups"""
    work = rows * (C // PIECE[dt])
    grid = min(max((work + NT - 1) // NT, 1), 4096)
    return (work + grid * NT - 1) // (grid * NT)


def rows_case(rows, C, dt, seed=0, extra=None):
    """`rows` unique logical rows out of rows + extra (rows // 3 + 2 unless given), in an order that is not monotonic; the physical matrix through ROW_MAP,
    ld = C + 8"""
    n_log = rows + (rows // 3 + 2 if extra is None else extra)
    rng = np.random.default_rng(seed + rows)
    idx = rng.permutation(n_log)[:rows].astype(np.int32)
    if rows > 2:
        assert (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    prow = phys_rows(n_log, ROW_MAP)
    nphys = int(prow.max()) + 1
    table = values(nphys, C, dt) if nphys <= 16384 else ints(nphys, C)         # (the second-trip cases have more rows than `coded` can tell apart)
    return NS(rows=rows, C=C, ld=C + 8, n_log=n_log, idx=idx, prow=prow, nphys=nphys, table=table, rmap=ROW_MAP)


def gather_ref(table, case, use_offset=True):
    """dst[r] = table[map(idx[r])]; use_offset=False: the gather that drops the map's offset"""
    rpb, stride, off = case.rmap
    p = (case.idx // rpb) * stride + (off if use_offset else 0) + case.idx % rpb
    return table[p]


def scatter_ref(dst, src, case, accumulate):
    """dst[map(idx[r])] (+)= src[r]; every other row keeps its value"""
    out = dst.copy()
    p = case.prow[case.idx]
    out[p] = dst[p] + src if accumulate else src
    return out


# ================================================================================================ masked_select
MS_ONE_PASS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536)
MS_LOOP = (65537, 66560)
MS_PATTERNS = ("none", "all", "lane63", "lane0", "last", "last_row")
MS_SENTINEL = 0x07070707


def ms_kernel(n):
    """mvlt_masked_select: one pass (at most 64 rows of 64 labels per wave) up to 65536 labels, the 1024-labels-per-trip loop beyond"""
    return "masked_select_kernel" if n <= 65536 else "masked_select_loop_kernel"


def ms_labels(n, pattern, ignore=-1, mixed=False):
    """labels [n]: `ignore` everywhere but the pattern's positions.  A 64-label row of the one-pass kernel starts at a multiple of 64 (a wave's first label
    is w * per * 64), so "lane l of every row" is p % 64 == l in both kernels.  mixed: the real labels include -1 (for an ignore_index other than -1)"""
    p = np.arange(n)
    sel = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "lane63": p % 64 == 63, "lane0": p % 64 == 0, "last": p == n - 1,
           "last_row": p >= ((n - 1) // 64) * 64, "random": (p * 2654435761 % 4294967296) % 5 < 2}[pattern]
    real = 5 + p % 7
    if mixed:
        real = np.where(p % 3 == 0, -1, real)
    return np.where(sel, real, ignore).astype(np.int64)


def ms_ref(labels, ignore):
    return np.nonzero(labels != ignore)[0].astype(np.int32)


def ms_drop_at_wave_boundary(idx):
    """the selection a kernel returns that loses the first selected label at or behind a wave boundary (position >= 64): everything behind it moves up"""
    k = int(np.argmax(idx >= 64))
    assert idx.size and idx[k] >= 64
    return np.delete(idx, k)


# ================================================================================================ row_scale
ROW_SCALE_SHAPES = ((1, 1, 8), (7, 3, 8), (130, 64, 64))      # (M, rows_per_scale, C): (7, 3): a ragged last sample; 130 x 64: 3 samples, the last of 2 rows
ROW_SCALE_FACTORS = (0.0, 0.5, 1.0, 2.0)


def row_scale_factors(M, rps):
    n = (M + rps - 1) // rps
    return np.array([ROW_SCALE_FACTORS[(i + M) % 4] for i in range(n)], dtype=np.float64)


def row_scale_ref(x, scale, rps):
    return x * scale[np.arange(x.shape[0]) // rps][:, None]


# ================================================================================================ head_grad_prep
HEAD_SHAPES = ((1, 2, 8), (3, 48, 48), (7, 122, 128), (300, 2, 8))        # (B, n, n_pad)
HEAD_DB1, HEAD_DB2 = 3.0, 5.0


def head_rstep(n_pad):
    """head_grad_prep_kernel: 256 threads = rstep row groups of n_pad columns -> (rstep, idle threads)"""
    return NT // n_pad, NT - (NT // n_pad) * n_pad


def head_ref(dlogits, n_pad):
    B, n = dlogits.shape
    dl = np.zeros((B, n_pad))
    dl[:, :n] = dlogits
    return dl, dlogits.sum(0)


# ================================================================================================ bilinear token resize
# source grid -> target grid
RESIZE_DYADIC = (((4, 4), (8, 8)), ((8, 8), (4, 4)), ((4, 8), (8, 4)), ((4, 4), (4, 4)), ((1, 1), (3, 5)), ((4, 4), (1, 8)))
RESIZE_OTHER = (((7, 7), (8, 6)), ((7, 7), (3, 5)), ((14, 14), (5, 20)))
RESIZE_C = (3, 64)
RESIZE_PREFILL = 5.0
U24 = 2.0 ** -24


def resize_axis(n_in, n_out):
    """source coordinates of one axis in float32, as the kernel states them: s = (float)n_in / (float)n_out, f = max(s * (o + 0.5f) - 0.5f, 0), i0 = (int)f,
    i1 = i0 + (i0 < n_in - 1), and the weight of i1 is f - i0 where there IS a neighbour, 0 where i1 is clamped onto i0 -> (i0, i1, l float32, clamped)"""
    s = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    f = np.maximum(s * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
    i0 = f.astype(np.int32)
    inner = i0 < n_in - 1
    l = np.where(inner, f - i0.astype(np.float32), np.float32(0.0)).astype(np.float32)
    return i0, i0 + inner, l, ~inner


def resize_terms(src, dst, clamp_x=True):
    """-> (idx [P, 4] source tokens, w [P, 4] float64 weights) of the P = hout * wout target pixels, corners in the kernel's order 00, 01, 10, 11.
    clamp_x=False: the kernel that forgets x1 = min(x0 + 1, Win - 1) -- it reads the next token (the first pixel of the next row; the last token stands in
    for what lies behind the map) with the weight fx - x0"""
    (hin, win), (hout, wout) = src, dst
    y0, y1, ly, _ = resize_axis(hin, hout)
    x0, x1, lx, xc = resize_axis(win, wout)
    lx = lx.astype(np.float64)
    if not clamp_x:
        s = np.float32(win) / np.float32(wout)
        f = np.maximum(s * (np.arange(wout, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0.0)).astype(np.float32)
        x1 = x0 + 1
        lx = (f - x0.astype(np.float32)).astype(np.float64)
    ly = ly.astype(np.float64)[:, None]
    lx = lx[None, :]
    tok = lambda yy, xx: np.minimum(yy[:, None] * win + xx[None, :], hin * win - 1)
    idx = np.stack([tok(y0, x0), tok(y0, x1), tok(y1, x0), tok(y1, x1)], -1).reshape(hout * wout, 4)
    w = np.stack([(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx], -1).reshape(hout * wout, 4)
    return idx, w


def resize_fwd_ref(x, idx, w):
    """x [hin * win, C] -> (out [P, C] float64, bar [P, C]); bar = 8 x 2^-24 x sum_k |w_k x_k|: the six roundings on the path of any term (1 - l, the
    product of two weights, the product with x, three additions) with margin for contraction"""
    terms = w[:, :, None] * x[idx]
    return terms.sum(1), 8 * U24 * np.abs(terms).sum(1)


def resize_adj_ref(g, idx, w, n_src, prefill):
    """g [P, C] -> (out [n_src, C] = prefill + A^T g in float64, bar): per scattered term 8 x 2^-24 x |w g|, summed over the contributors of the element,
    plus n_contrib x 2^-24 x |sum| for the atomic additions (n_contrib counts the terms of non-zero weight; with g >= 0 and prefill >= 0 every partial sum
    is at most the final one)"""
    C = g.shape[1]
    out, absum, cnt = np.full((n_src, C), float(prefill)), np.zeros((n_src, C)), np.zeros((n_src, 1))
    for k in range(4):
        np.add.at(out, idx[:, k], w[:, k, None] * g)
        np.add.at(absum, idx[:, k], np.abs(w[:, k, None] * g))
        np.add.at(cnt, idx[:, k], (w[:, k, None] != 0).astype(np.float64))
    return out, 8 * U24 * absum + cnt * U24 * np.abs(out)


def resize_input(tokens, C, seed=0):
    """positive integers below 2^12 that tell tokens and channels apart"""
    v = (np.arange(tokens)[:, None] * 67 + np.arange(C)[None, :] * 29 + 1 + seed) % 4093 + 1
    assert v.max() < 2 ** 12 and v.min() >= 1
    return v.astype(np.float64)


def resize_is_dyadic(idx, w):
    return bool(np.all(w * 16 == np.round(w * 16)))
