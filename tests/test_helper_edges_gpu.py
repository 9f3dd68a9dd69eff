"""GPU: the layout and index helper kernels of csrc/elementwise.hip -- weight_prep, transpose_cast, patchify / patchify_strip, gather_rows / scatter_rows,
masked_select / masked_select_loop, row_scale, head_grad_prep, resize_tokens / resize_tokens_multi -- against the numpy / float64 references of
tests/helper_cases.py, at the shapes where a tile bound, a lookup path, a wave boundary or a clamped index can go wrong.  The premises of the inputs are
pinned on the CPU by tests/test_helper_cases_cpu.py; docs/helper_edges.md maps every case to the instantiation and the branch it reaches.

Everything except a non-dyadic resize is data movement and is compared BIT FOR BIT: the float64 reference rounded once to the output dtype.

EVERY launch goes through `launch`: operands and results live in flat device buffers filled with the sentinel 7.0 (integers: 0x07070707), with gap columns
wherever the entry point takes a leading dimension and a guard row (or guard elements) behind every buffer.  After the launch the WHOLE buffer -- results,
gaps and guards in one array -- is compared with the expected image, every operand buffer with what was uploaded, and the name of the instantiation that
mvlt_amd._lib.last_kernel() reports with the one the case is there for.

Bars exist only for the non-dyadic resizes (helper_cases.resize_fwd_ref / resize_adj_ref): per element 8 x 2^-24 x sum |w x| forward; the same per
scattered term plus n_contrib x 2^-24 x |sum| for the atomic additions of the adjoint.  The achieved error / bar goes through the `parity` fixture.
"""
import numpy as np
import pytest
import torch

from tests import helper_cases as hc

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
TD = {"bf16": BF, "fp32": F32}
ESIZE = {BF: 2, F32: 4}
GUARD = 64                                       # guard elements behind a buffer that has no rows


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from mvlt_amd import ops as _ops
    return _ops


def last_kernel():
    from mvlt_amd._lib import last_kernel as lk
    return lk()


def ran(base, *targs):
    """the kernel launched last on this thread must be the instantiation base<targs> (a dtype or a bool).  An instantiation over the bf16 element type
    comes back mangled (the C++ runtime's demangler does not know that type): the template arguments are looked up in the mangled form then."""
    name = last_kernel()
    if not targs:
        assert name == base, f"meant to reach {base}, the library launched {name}"
    elif name.startswith("_Z"):
        enc = lambda t: "DF16b" if t is BF else "f" if t is F32 else f"Lb{int(t)}E"
        want = f"{len(base)}{base}I" + "".join(enc(t) for t in targs) + "E"
        assert want in name, f"meant to reach {base}{targs} ({want}), the library launched {name}"
    else:
        txt = lambda t: "float" if t is F32 else str(t).lower()
        want = f"{base}<" + ", ".join(txt(t) for t in targs) + ">"
        assert name == want, f"meant to reach {want}, the library launched {name}"


# ------------------------------------------------------------------------------------------------ buffers, guards, the one launch helper
class Flat:
    """a flat device buffer uploaded from its host image (float64 values -> dtype, exactly or rounded once; or an integer array as it is); the image
    includes the sentinels of the gaps and guards"""

    def __init__(self, image, dtype):
        self.dtype = dtype
        if dtype in TD.values():
            self.h0 = hc.as_stored(image, "bf16" if dtype is BF else "fp32")
            self.t = torch.from_numpy(self.h0).to(dev()).to(dtype)
        else:
            self.h0 = np.ascontiguousarray(image, dtype={torch.int32: np.int32, torch.int64: np.int64}[dtype])
            self.t = torch.from_numpy(self.h0).to(dev())
        assert self.t.data_ptr() % 16 == 0

    def host(self):
        return (self.t.float() if self.dtype is BF else self.t).cpu().numpy()


def sentinels(n):
    return np.full(n, hc.SENTINEL)


def lay(dense, ld, prow=None, nphys=None, fill=hc.SENTINEL):
    """host image of a [rows, C] matrix whose rows are ld apart, logical row r at physical row prow[r], with one guard row: gaps and guard are sentinels;
    physical rows that hold no logical row are `fill`"""
    rows, C = dense.shape
    prow = np.arange(rows) if prow is None else prow
    nphys = nphys or int(prow.max()) + 1
    img = np.full((nphys + 1, ld), hc.SENTINEL)
    img[:nphys, :C] = fill
    img[prow, :C] = dense
    return img.reshape(-1)


def launch(what, call, kernel, ins=(), outs=()):
    """run `call`, assert the instantiation it launched, then compare every output buffer in full -- values, gap columns, guards -- with its expected image
    and every operand buffer with what was uploaded, bit for bit.  outs: (name, Flat, expected float64 image, dt or None for integers[, mask of the
    elements to compare: the rest is judged against a bar by the caller])"""
    call()
    ran(*kernel)
    torch.cuda.synchronize()
    for name, b in ins:
        msg = hc.mismatch(b.host(), b.h0)
        assert msg is None, f"{what}: the operand {name} was written: {msg}; last kernel {last_kernel()}"
    for name, b, want, dt, *where in outs:
        want = hc.as_stored(want, dt) if dt else np.asarray(want, dtype=b.h0.dtype)
        msg = hc.mismatch(b.host(), want, *where)
        assert msg is None, f"{what}: {name}: {msg}; last kernel {last_kernel()}"


def refused(call, *untouched):
    """an argument check that returns before any launch: MVLTError, the last kernel's name unchanged, nothing written"""
    from mvlt_amd._lib import MVLTError
    before = last_kernel()
    with pytest.raises(MVLTError):
        call()
    torch.cuda.synchronize()
    assert last_kernel() == before
    for b in untouched:
        msg = hc.mismatch(b.host(), b.h0)
        assert msg is None, f"a refused call wrote: {msg}"


def judge(parity, name, what, got, ref, bar):
    ratio = np.abs(got.astype(np.float64) - ref) / np.maximum(bar, 1e-300)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert parity(f"{name}/{what}", ratio.max(), 1.0), (f"{what}: {name} element {tuple(int(i) for i in at)}: got {got[at]!r}, want {ref[at]!r}, bar {bar[at]:.3e} "
                                                       f"({ratio[at]:.2f} bars); last kernel {last_kernel()}")
    return float(ratio.max())


# ================================================================================================ weight_prep
def run_prep(ops, case):
    from mvlt_amd import params
    from mvlt_amd._lib import PrepDesc
    T = TD[case.dt]
    srcs = [Flat(np.concatenate([s, sentinels(GUARD)]), TD[sdt]) for s, sdt in case.srcs]
    refs = hc.prep_ref(case)
    images = []
    for n, (want, wr) in zip(case.dst_sizes, refs):
        img = sentinels(n + GUARD)
        img[:n][wr] = want[wr]
        images.append(img)
    results = {}
    for path in ("blk_desc", "search"):
        dsts = [Flat(sentinels(n + GUARD), T) for n in case.dst_sizes]
        descs = [PrepDesc(srcs[d.src[0]].t.data_ptr() + d.src[1] * ESIZE[srcs[d.src[0]].dtype], dsts[d.dst[0]].t.data_ptr() + d.dst[1] * ESIZE[T], d.kind,
                          d.R, d.C, d.ld_out, d.d0, d.d1, d.d2, d.src_off, d.ss0, d.ss1, d.ss2, d.ds0, d.ds1, d.ds2) for d in case.descs]
        tab, blk, ndesc, total, blk_desc = params.pack_prep_table(descs, T, dev())
        assert ndesc == len(case.descs) and total == sum(hc.prep_blocks(d) for d in case.descs) and blk_desc.numel() == total
        launch(f"weight_prep {case.name} {case.dt} {path}", lambda: ops.weight_prep(tab, blk, ndesc, total, T, blk_desc if path == "blk_desc" else None),
               ("weight_prep_kernel", T), ins=[(f"src{k}", s) for k, s in enumerate(srcs)],
               outs=[(f"dst{k}", b, images[k], case.dt) for k, b in enumerate(dsts)])
        results[path] = dsts
    for a, b in zip(results["blk_desc"], results["search"]):
        assert torch.equal(a.t.view(torch.int16 if T is BF else torch.int32), b.t.view(torch.int16 if T is BF else torch.int32)), "both lookup paths, the same bits"


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_weight_prep_single_descriptors(ops, dt):
    """every kind 0 shape at ld_out = R and R + 5 (the padding columns keep the sentinel), every kind 2 shape (bf16: zeros up to min(ld_out, tile edge), the
    sentinel beyond), the 255 / 256 / 257-element gathers, the flipped taps and the conv permutation, each on both lookup paths"""
    for case in hc.prep_single_cases(dt):
        run_prep(ops, case)


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_weight_prep_mixed_table(ops, dt):
    run_prep(ops, hc.prep_mixed_case(dt))


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_weight_prep_1025_descriptors_search_in_global_memory(ops, dt):
    case = hc.prep_many_case(dt)
    assert hc.prep_search(len(case.descs)) == "global"
    run_prep(ops, case)


def test_weight_prep_table_refuses_kind_2_with_an_fp32_destination():
    """a kind-2 descriptor compiles to nothing in the fp32 instantiation: the table builder that owns the table refuses it (the C entry point cannot read a
    device table), and it refuses a kind-2 shape off the 16-byte grid"""
    from mvlt_amd import params
    from mvlt_amd._lib import MVLTError, PrepDesc
    src, dst = Flat(sentinels(64 * 64 + GUARD), BF), Flat(sentinels(64 * 64 + GUARD), F32)
    d = lambda kind, R, C, ld: PrepDesc(src.t.data_ptr(), dst.t.data_ptr(), kind, R, C, ld, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    before = last_kernel()
    with pytest.raises(MVLTError, match="kind 2"):
        params.pack_prep_table([d(0, 8, 8, 8), d(2, 64, 64, 64)], F32, dev())
    with pytest.raises(MVLTError, match="multiples of 8"):
        params.pack_prep_table([d(2, 60, 36, 64)], BF, dev())
    with pytest.raises(MVLTError, match="ld_out"):
        params.pack_prep_table([d(0, 9, 8, 8)], F32, dev())
    assert last_kernel() == before
    assert params.pack_prep_table([d(2, 64, 64, 64)], BF, dev())[2] == 1


# ================================================================================================ transpose_cast
@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("R,C", hc.TRANSPOSE_SHAPES, ids=lambda v: str(v))
def test_transpose_cast_smallest_shapes(ops, R, C, dt):
    T, ld = TD[dt], R + 5
    x = hc.fracs(R, C)
    w = Flat(np.concatenate([x.reshape(-1), sentinels(GUARD)]), F32)
    out = Flat(sentinels((C + 1) * ld), T)
    launch(f"transpose_cast {R}x{C}", lambda: ops.transpose_cast(w.t, out.t, R, C, ld), ("transpose_cast_kernel", T), ins=[("w", w)],
           outs=[("out", out, lay(hc.transpose_ref(x), ld), dt)])


# ================================================================================================ patchify
@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("case", hc.PATCHIFY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_patchify(ops, case, dt):
    """P == unfold(img) rounded once, in every bit: the generic kernel at (k, Cin) = (2, 8), (8, 1), (4, 4), through a misaligned `out` and past the LDS limit
    at the model's (4, 3); the strip kernel at one patch, at its widest strip and over several samples"""
    k, Cin, B, H, W, off, route = case
    T = TD[dt]
    x = hc.patchify_image(B, Cin, H, W, dt)
    ref = hc.patchify_ref(x, k)
    rows, K = ref.shape
    img = Flat(np.concatenate([x.reshape(-1), sentinels(GUARD)]), F32)
    out = Flat(sentinels(off + rows * K + K), T)
    view = out.t[off:]
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    want = np.concatenate([sentinels(off), ref.reshape(-1), sentinels(K)])
    launch(f"patchify k{k} Cin{Cin} {B}x{H}x{W} +{off}", lambda: ops.patchify(img.t, view, B, Cin, H, W, k),
           ("patchify_strip_kernel" if route == "strip" else "patchify_kernel", T), ins=[("img", img)], outs=[("P", out, want, dt)])


# ================================================================================================ gather / scatter
def rowmap(case):
    from mvlt_amd._lib import rowmap as make
    return make(*case.rmap)


def idx_buf(case):
    return Flat(np.concatenate([case.idx, [hc.MS_SENTINEL]]), torch.int32)


def run_gather(ops, what, case, dt):
    T = TD[dt]
    src = Flat(lay(case.table, case.ld), T)
    idx = idx_buf(case)
    dst = Flat(sentinels((case.rows + 1) * case.C), T)
    launch(what, lambda: ops.gather_rows(src.t, idx.t, dst.t, case.rows, case.C, case.ld, rowmap(case)), ("gather_rows_kernel", T),
           ins=[("src", src), ("idx", idx)], outs=[("dst", dst, lay(hc.gather_ref(case.table, case), case.C), dt)])


def run_scatter(ops, what, case, dt, accumulate):
    T = TD[dt]
    vals = hc.ints(case.rows, case.C, mod=113)
    src = Flat(lay(vals, case.C), T)
    idx = idx_buf(case)
    dst = Flat(lay(case.table, case.ld), T)
    launch(what, lambda: ops.scatter_rows(src.t, idx.t, dst.t, case.rows, case.C, case.ld, rowmap(case), accumulate=accumulate), ("scatter_rows_kernel", T),
           ins=[("src", src), ("idx", idx)], outs=[("dst", dst, lay(hc.scatter_ref(case.table, vals, case, accumulate), case.ld), dt)])


@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("rows,wide", hc.ROWS_CASES, ids=lambda v: str(v))
def test_gather_scatter_rows(ops, rows, wide, dt):
    """one 16-byte piece per row and C = 520, ld = C + 8, a row map with rows_per_batch, batch_stride and offset, idx not monotonic.  The scatter runs on a
    non-zero destination of integers, accumulate 0 and 1: the rows idx does not name, the gap columns and the guard row keep their bits"""
    C = 520 if wide else hc.PIECE[dt]
    case = hc.rows_case(rows, C, dt)
    assert hc.row_trips(rows, C, dt) == 1
    run_gather(ops, f"gather {rows}x{C}", case, dt)
    for acc in (False, True):
        run_scatter(ops, f"scatter {rows}x{C} accumulate={acc}", case, dt, acc)


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_gather_scatter_second_grid_stride_trip(ops, dt):
    """more 16-byte pieces than 4096 workgroups x 256 threads take in one trip"""
    rows = hc.ROWS_SECOND_TRIP[dt]
    case = hc.rows_case(rows, 520, dt, extra=7)
    assert hc.row_trips(rows, 520, dt) == 2
    run_gather(ops, f"gather {rows}x520", case, dt)
    run_scatter(ops, f"scatter {rows}x520 accumulate", case, dt, True)


@pytest.mark.parametrize("dt", hc.DTYPES)
def test_gather_scatter_refusals(ops, dt):
    """C that is no multiple of the 16-byte piece; a row map whose mode is not 0 (patch and 3x3-neighbourhood maps belong to the GEMM entry points)"""
    from mvlt_amd._lib import conv3map, patchmap
    T, pc = TD[dt], hc.PIECE[dt]
    case = hc.rows_case(5, 2 * pc, dt)
    src, idx = Flat(lay(case.table, case.ld), T), idx_buf(case)
    dst = Flat(sentinels(6 * case.C), T)
    big = Flat(lay(case.table, case.ld), T)
    refused(lambda: ops.gather_rows(src.t, idx.t, dst.t, 5, case.C - pc // 2, case.ld, rowmap(case)), dst)
    refused(lambda: ops.scatter_rows(dst.t, idx.t, big.t, 5, case.C - pc // 2, case.ld, rowmap(case)), big)
    for m in (patchmap(2, 4, 16, 4, 2, case.C), conv3map(2, 2, 4, case.C)):
        refused(lambda: ops.gather_rows(src.t, idx.t, dst.t, 5, case.C, case.ld, m), dst)
        refused(lambda: ops.scatter_rows(dst.t, idx.t, big.t, 5, case.C, case.ld, m), big)
        refused(lambda: ops.scatter_rows(dst.t, idx.t, big.t, 5, case.C, case.ld, m, accumulate=True), big)


# ================================================================================================ masked_select
def run_select(ops, what, labels, ignore):
    from mvlt_amd import _lib as L
    n = labels.size
    want = hc.ms_ref(labels, ignore)
    lab = Flat(np.concatenate([labels, [3]]), torch.int64)                       # the guard label is a REAL label: a read past n would select it
    idx = Flat(np.full(n + 2, hc.MS_SENTINEL), torch.int32)                      # n + 1 entries and a guard
    cnt = Flat(np.full(2, hc.MS_SENTINEL), torch.int32)
    img = np.full(n + 2, hc.MS_SENTINEL)
    img[:want.size] = want
    if n:
        call = lambda: ops.masked_select(lab.t[:n], idx.t, cnt.t, ignore_index=ignore)
    else:                                                                        # (an empty tensor has no address: the entry point itself, n = 0)
        call = lambda: L.check(L.lib.mvlt_masked_select(L.ptr(lab.t), 0, ignore, L.ptr(idx.t), L.ptr(cnt.t), L.stream_ptr()), "mvlt_masked_select")
    launch(what, call, (hc.ms_kernel(n),), ins=[("labels", lab)], outs=[("idx", idx, img, None), ("count", cnt, [want.size, hc.MS_SENTINEL], None)])


@pytest.mark.parametrize("n", hc.MS_ONE_PASS + hc.MS_LOOP)
def test_masked_select(ops, n):
    """none, all, only lane 63 / only lane 0 of every 64-label row, only the last label, only the last (partial) row; ignore_index = -100 with -1 a real
    label.  idx[count:] and the guard keep the sentinel, count is exact"""
    for pat in hc.MS_PATTERNS:
        run_select(ops, f"masked_select n{n} {pat}", hc.ms_labels(n, pat), -1)
    run_select(ops, f"masked_select n{n} ignore -100", hc.ms_labels(n, "random", ignore=-100, mixed=True), -100)
    run_select(ops, f"masked_select n{n} random", hc.ms_labels(n, "random"), -1)


# ================================================================================================ row_scale
@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("M,rps,C", hc.ROW_SCALE_SHAPES, ids=lambda v: str(v))
def test_row_scale(ops, M, rps, C, dt):
    T = TD[dt]
    x, s = hc.values(M, C, dt), hc.row_scale_factors(M, rps)
    xb, sb = Flat(lay(x, C), T), Flat(np.concatenate([s, sentinels(1)]), F32)
    out = Flat(sentinels((M + 1) * C), T)
    launch(f"row_scale {M}x{C} per {rps}", lambda: ops.row_scale(xb.t, sb.t, rps, M, C, out.t), ("row_scale_kernel", T), ins=[("x", xb), ("scale", sb)],
           outs=[("out", out, lay(hc.row_scale_ref(x, s, rps), C), dt)])


# ================================================================================================ head_grad_prep
@pytest.mark.parametrize("dt", hc.DTYPES)
@pytest.mark.parametrize("two", [True, False], ids=["db2", "db2-null"])
@pytest.mark.parametrize("B,n,n_pad", hc.HEAD_SHAPES, ids=lambda v: str(v))
def test_head_grad_prep(ops, B, n, n_pad, two, dt):
    """n_pad = 48: rstep = 5 and 16 idle threads; B = 1 below rstep, B = 300 many trips; db1 starts at 3, db2 at 5 or is NULL"""
    T = TD[dt]
    d = hc.ints(B, n)
    dl_ref, sums = hc.head_ref(d, n_pad)
    dlog = Flat(lay(d, n), F32)
    dl = Flat(sentinels((B + 1) * n_pad), T)
    db1 = Flat(np.concatenate([np.full(n, hc.HEAD_DB1), sentinels(1)]), F32)
    db2 = Flat(np.concatenate([np.full(n, hc.HEAD_DB2), sentinels(1)]), F32)
    outs = [("dl", dl, lay(dl_ref, n_pad), dt), ("db1", db1, np.concatenate([hc.HEAD_DB1 + sums, sentinels(1)]), "fp32"),
            ("db2", db2, np.concatenate([hc.HEAD_DB2 + (sums if two else np.zeros(n)), sentinels(1)]), "fp32")]
    launch(f"head_grad_prep B{B} n{n} n_pad{n_pad}", lambda: ops.head_grad_prep(dlog.t[:B * n].view(B, n), dl.t[:B * n_pad].view(B, n_pad), db1.t[:n],
                                                                                 db2.t[:n] if two else None),
           ("head_grad_prep_kernel", T), ins=[("dlogits", dlog)], outs=outs)


# ================================================================================================ bilinear token resize
RESIZE_ALL = [(s, d, True) for s, d in hc.RESIZE_DYADIC] + [(s, d, False) for s, d in hc.RESIZE_OTHER]
RESIZE_IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d, _ in RESIZE_ALL]


class ResizeJob:
    """operands, buffers and references of one (source grid -> target grid, C) resize: the forward reads x [n_src, C] (rows C + 3 apart) into y [P, C] (rows
    C + 5 apart); the adjoint reads g [P, C] (rows C + 5 apart) into dx [n_src, C] (rows C + 5 apart), pre-filled with 5"""

    def __init__(self, src, dst, C, dyadic):
        self.src, self.dst, self.C, self.dyadic = src, dst, C, dyadic
        self.n_src, self.P = src[0] * src[1], dst[0] * dst[1]
        self.idx, self.w = hc.resize_terms(src, dst)
        self.x, self.g = hc.resize_input(self.n_src, C), hc.resize_input(self.P, C, seed=7)
        self.y_ref, self.y_bar = hc.resize_fwd_ref(self.x, self.idx, self.w)
        self.dx_ref, self.dx_bar = hc.resize_adj_ref(self.g, self.idx, self.w, self.n_src, hc.RESIZE_PREFILL)
        self.tag = f"{src[0]}x{src[1]}->{dst[0]}x{dst[1]} C{C}"
        self.fresh()

    def fresh(self):
        C = self.C
        self.xb, self.gb = Flat(lay(self.x, C + 3), F32), Flat(lay(self.g, C + 5), F32)
        self.yb = Flat(sentinels((self.P + 1) * (C + 5)), F32)
        self.dxb = Flat(lay(np.full((self.n_src, C), hc.RESIZE_PREFILL), C + 5), F32)

    def view(self, b, rows, ld):
        return b.t[:rows * ld].view(rows, ld)[:, :self.C]

    def fwd_args(self):
        return (self.view(self.xb, self.n_src, self.C + 3), self.view(self.yb, self.P, self.C + 5), *self.src, *self.dst, self.C)

    def adj_args(self):
        return (self.view(self.gb, self.P, self.C + 5), self.view(self.dxb, self.n_src, self.C + 5), *self.src, *self.dst, self.C)

    def live(self, rows, ld):
        m = np.zeros((rows + 1, ld), dtype=bool)
        m[:rows, :self.C] = True
        return m.reshape(-1)

    def outs(self, adjoint):
        """the expected image of y or dx: exact in a dyadic case; otherwise only the gaps and the guard are exact and the caller judges the rest"""
        rows, ld, ref, b, name = (self.n_src, self.C + 5, self.dx_ref, self.dxb, "dx") if adjoint else (self.P, self.C + 5, self.y_ref, self.yb, "y")
        if self.dyadic:
            return [(name, b, lay(ref, ld), "fp32")]
        return [(name, b, lay(np.zeros_like(ref), ld), "fp32", ~self.live(rows, ld))]

    def dense(self, adjoint):
        rows, ld, b = (self.n_src, self.C + 5, self.dxb) if adjoint else (self.P, self.C + 5, self.yb)
        return b.host()[:rows * ld].reshape(rows, ld)[:, :self.C]

    def judge(self, parity, what, adjoint):
        if not self.dyadic:
            ref, bar = (self.dx_ref, self.dx_bar) if adjoint else (self.y_ref, self.y_bar)
            judge(parity, f"resize {'adjoint' if adjoint else 'forward'} {self.tag}", what, self.dense(adjoint), ref, bar)

    def ins(self, adjoint):
        return [("g", self.gb)] if adjoint else [("x", self.xb)]


@pytest.mark.parametrize("C", hc.RESIZE_C)
@pytest.mark.parametrize("src,dst,dyadic", RESIZE_ALL, ids=RESIZE_IDS)
def test_resize_forward_adjoint_and_identity(ops, parity, src, dst, dyadic, C):
    """forward and adjoint of one resize through mvlt_resize_bilinear_tokens, ld_out = C + 5 with guard columns, the adjoint onto a destination that holds 5;
    the dyadic cases (enlarging, shrinking, mixed, the identity size -- a copy --, a 1 x 1 source, a one-row target) in every bit; then
    <A x, g> == <x, A^T g> in float64 on the GPU's results: exactly for the dyadic cases, within the two bars otherwise"""
    j = ResizeJob(src, dst, C, dyadic)
    launch(f"resize forward {j.tag}", lambda: ops.resize_bilinear_tokens(*j.fwd_args()), ("resize_tokens_kernel", False), ins=j.ins(False), outs=j.outs(False))
    j.judge(parity, "single", False)
    launch(f"resize adjoint {j.tag}", lambda: ops.resize_bilinear_tokens(*j.adj_args(), adjoint=True), ("resize_tokens_kernel", True), ins=j.ins(True),
           outs=j.outs(True))
    j.judge(parity, "single", True)
    y, dx = j.dense(False).astype(np.float64), j.dense(True).astype(np.float64) - hc.RESIZE_PREFILL
    if src == dst:
        assert hc.mismatch(j.dense(False), j.x.astype(np.float32)) is None, "the identity size is a copy"
    lhs, rhs = float((y * j.g).sum()), float((j.x * dx).sum())
    if dyadic:
        assert lhs == rhs, f"<A x, g> = {lhs!r}, <x, A^T g> = {rhs!r}"
    else:
        bar = float((j.y_bar * j.g).sum() + (j.x * j.dx_bar).sum())
        assert parity(f"resize adjoint identity {j.tag}", abs(lhs - rhs), bar), f"<A x, g> = {lhs!r}, <x, A^T g> = {rhs!r}, bar {bar:.3e}"


MULTI_SETS = {
    "one-dyadic": [((4, 4), (8, 8), 64, True)],
    "one-other": [((14, 14), (5, 20), 3, False)],
    "four": [((1, 1), (3, 5), 3, True), ((14, 14), (5, 20), 64, False), ((8, 8), (4, 4), 64, True), ((7, 7), (8, 6), 3, False)],
}


@pytest.mark.parametrize("which", list(MULTI_SETS))
def test_resize_multi_launch(ops, parity, which):
    """1 job and 4 jobs of very different sizes (15 x 3 elements next to 100 x 64: the grid is sized for the largest) in one launch: every forward is
    torch.equal to its single launch, every dyadic adjoint too, the other adjoints are within their bar"""
    jobs = [ResizeJob(*spec) for spec in MULTI_SETS[which]]
    single = []
    for j in jobs:
        ops.resize_bilinear_tokens(*j.fwd_args())
        ops.resize_bilinear_tokens(*j.adj_args(), adjoint=True)
        torch.cuda.synchronize()
        single.append((j.yb.t.clone(), j.dxb.t.clone()))
        j.fresh()
    launch(f"resize multi forward {which}", lambda: ops.resize_bilinear_tokens_multi([j.fwd_args() for j in jobs]), ("resize_tokens_multi_kernel", False),
           ins=[i for j in jobs for i in j.ins(False)], outs=[o for j in jobs for o in j.outs(False)])
    launch(f"resize multi adjoint {which}", lambda: ops.resize_bilinear_tokens_multi([j.adj_args() for j in jobs], adjoint=True),
           ("resize_tokens_multi_kernel", True), ins=[i for j in jobs for i in j.ins(True)], outs=[o for j in jobs for o in j.outs(True)])
    for j, (y1, dx1) in zip(jobs, single):
        assert torch.equal(j.yb.t.view(torch.int32), y1.view(torch.int32)), f"{j.tag}: the multi launch's forward differs from the single launch"
        j.judge(parity, f"multi {which}", False)
        j.judge(parity, f"multi {which}", True)
        if j.dyadic:
            assert torch.equal(j.dxb.t.view(torch.int32), dx1.view(torch.int32)), f"{j.tag}: the multi launch's adjoint differs from the single launch"


def test_resize_multi_refuses_0_and_5_jobs(ops):
    from mvlt_amd import _lib as L
    import ctypes as C
    j = ResizeJob((4, 4), (8, 8), 3, True)
    before = last_kernel()
    for n in (0, 5):
        with pytest.raises((AssertionError, L.MVLTError)):
            ops.resize_bilinear_tokens_multi([j.fwd_args()] * n)
        # the entry point itself (ops asserts before it gets there)
        k = max(n, 1)
        P, I = C.c_void_p * k, C.c_int * k
        a = j.fwd_args()
        rc = L.lib.mvlt_resize_bilinear_tokens_multi(P(*[L.ptr(a[0])] * k), I(*[j.C + 3] * k), P(*[L.ptr(a[1])] * k), I(*[j.C + 5] * k), I(*[4] * k), I(*[4] * k),
                                                     I(*[8] * k), I(*[8] * k), I(*[3] * k), n, 0, L.stream_ptr())
        assert rc != 0 and "1..4" in L.lib.mvlt_last_error().decode()
    torch.cuda.synchronize()
    assert last_kernel() == before
    assert hc.mismatch(j.yb.host(), j.yb.h0) is None
