"""CPU: the premises of the helper-kernel cases (tests/helper_cases.py) that tests/test_helper_edges_gpu.py runs on the GPU.  Pinned here: the one
rounding of the references against torch's own, the exactness premises (integral references below 2^24, dyadic resize weights, unique index sets), the
references against torch's operators where torch has one, and that every case reaches the branch it is there for -- the host dispatch conditions of
csrc/elementwise.hip are restated in helper_cases (patchify_route, ms_kernel, prep_search, head_rstep, row_trips).  Then each reference is perturbed the
way a wrong kernel would be wrong, and the comparison the GPU file uses must fail and name the element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helper_cases as hc


def fails_naming(got, want, at=None, where=None):
    """the GPU file's comparison must fail on `got` and say where; -> the message"""
    msg = hc.mismatch(np.asarray(got, dtype=want.dtype), want, where)
    assert msg is not None and "first at element" in msg, msg
    if at is not None:
        assert f"first at element {tuple(at)}" in msg, msg
    return msg


# ------------------------------------------------------------------------------------------------ rounding and values
def test_the_one_rounding_is_torchs_bf16_rounding():
    x = np.concatenate([hc.fracs(130, 136).reshape(-1), hc.patchify_image(1, 3, 8, 1360, "bf16").reshape(-1), [0.0, -0.0, 1.00390625, 1.01171875, 257.0, 255.5]])
    want = torch.from_numpy(x).float().to(torch.bfloat16).double().numpy()
    assert np.array_equal(hc.bf16_round(x), want)
    assert (hc.bf16_round(x) != x).mean() > 0.3, "the rounded values must show their rounding"
    assert np.array_equal(hc.bf16_round(hc.ints(130, 136)), hc.ints(130, 136)), "ints are exact in bf16"
    two = hc.ints(64, 64) + hc.ints(64, 64, mod=113)
    assert np.array_equal(hc.bf16_round(two), two), "and so are their pairwise sums"
    with pytest.raises(AssertionError):
        hc.bf16_round(np.array([0.1]))


def test_values_tell_positions_apart():
    c = hc.coded(130, 136)
    assert np.unique(c).size == c.size and c.max() < 2 ** 24
    for v in (hc.ints(130, 136), hc.fracs(130, 136)):
        assert (v[:, 1:] != v[:, :-1]).all() and (v[1:] != v[:-1]).all()
        sq = v[:64, :64]
        off = ~np.eye(64, dtype=bool)
        assert (sq != sq.T)[off].mean() > 0.95


# ------------------------------------------------------------------------------------------------ weight_prep
@pytest.mark.parametrize("dt", hc.DTYPES)
def test_weight_prep_tables(dt):
    singles = hc.prep_single_cases(dt)
    names = [c.name for c in singles]
    assert len(set(names)) == len(names)
    for R, C in hc.PREP_T0:
        assert f"kind0-{R}x{C}-ld{R}" in names and f"kind0-{R}x{C}-ld{R + 5}" in names
    assert any(R % 64 and C % 64 for R, C in hc.PREP_T0) and (64, 64) in hc.PREP_T0
    assert ("kind2-60x72-ld64" in names) == (dt == "bf16"), "kind 2 exists only with a bf16 destination"
    for n in (255, 256, 257):
        case = singles[names.index(f"kind1-n{n}")]
        d = case.descs[0]
        assert d.d0 * d.d1 * d.d2 == n and hc.prep_blocks(d) == (n + 255) // 256
    assert singles[names.index("kind1-flipped")].descs[0].ss1 < 0
    for case in singles + [hc.prep_mixed_case(dt), hc.prep_many_case(dt)]:
        for (want, wr), n in zip(hc.prep_ref(case), case.dst_sizes):
            hc.as_stored(want, dt)                                            # exact in fp32; rounded once for bf16
            assert wr.any() and want.shape == (n,)
        for src, sdt in case.srcs:
            assert np.array_equal(hc.as_stored(src, sdt).astype(np.float64), src), "sources are exact as stored"
        for d in case.descs:
            if d.kind == 2:
                assert d.C % 8 == 0 and d.ld_out % 8 == 0 and dt == "bf16"
    mixed = hc.prep_mixed_case(dt)
    assert {d.kind for d in mixed.descs} == ({0, 1, 2} if dt == "bf16" else {0, 1})
    starts = np.cumsum([0] + [hc.prep_blocks(d) for d in mixed.descs])[:-1]
    assert any(s % hc.prep_blocks(d) for s, d in zip(starts[1:], mixed.descs[1:]))
    assert hc.prep_search(len(mixed.descs)) == "lds"
    many = hc.prep_many_case(dt)
    assert len(many.descs) == 1025 and hc.prep_search(1025) == "global" and hc.prep_search(1024) == "lds"
    assert all(hc.prep_blocks(d) == 1 for d in many.descs)
    assert len({d.dst[1] for d in many.descs}) == 1025 and len({d.src[1] for d in many.descs}) == 1025


def test_weight_prep_padding_columns():
    """kind 0 writes exactly R columns of a row of W^T; kind 2 whole 16-byte pieces: zeros in [R, min(ld_out, tile edge)), nothing beyond"""
    got = {(R, C, ld): hc.prep_written_cols(hc.desc(2, (0, 0), (0, 0), R=R, C=C, ld_out=ld)) for R, C, ld in hc.PREP_T2}
    assert got == {(64, 64, 64): 64, (60, 72, 64): 64, (8, 136, 16): 16, (64, 8, 72): 64}
    assert hc.prep_written_cols(hc.desc(0, (0, 0), (0, 0), R=63, C=65, ld_out=68)) == 63
    case = [c for c in hc.prep_single_cases("bf16") if c.name == "kind2-60x72-ld64"][0]
    want, wr = hc.prep_ref(case)[0]
    want, wr = want.reshape(72, 64), wr.reshape(72, 64)
    assert wr.all() and (want[:, 60:] == 0).all() and np.array_equal(want[:, :60], hc.ints(60, 72).T)
    case = [c for c in hc.prep_single_cases("bf16") if c.name == "kind2-64x8-ld72"][0]
    assert not hc.prep_ref(case)[0][1].reshape(8, 72)[:, 64:].any()


def test_gather_references_are_the_torch_permutations():
    g = hc.prep_gather_parts("fp32")
    kind, src, size, kw = g["permute"]
    case = hc._prep_case("p", "fp32", [g["permute"]])
    want = torch.from_numpy(src[:4 * 3 * 4]).view(4, 3, 2, 2).permute(0, 2, 3, 1).reshape(-1).numpy()
    assert np.array_equal(hc.prep_ref(case)[0][0], want)
    kind, src, size, kw = g["flipped"]
    case = hc._prep_case("f", "fp32", [g["flipped"]])
    want = torch.from_numpy(src).view(5, 3, 9).flip(-1).permute(1, 2, 0).reshape(-1).numpy()           # [cin][8 - t][out]
    assert np.array_equal(hc.prep_ref(case)[0][0], want)


# ------------------------------------------------------------------------------------------------ transposes: the two ways of getting a tile wrong
@pytest.mark.parametrize("T,R,C", [(64, 65, 63), (64, 130, 7), (32, 33, 1)])
def test_transpose_perturbations(T, R, C):
    x = hc.fracs(R, C)
    want = hc.as_stored(hc.transpose_ref(x), "bf16")
    stored = lambda a: np.where(np.isnan(a), np.float32(np.nan), hc.as_stored(np.nan_to_num(a), "bf16"))      # NaN: never written
    assert hc.mismatch(hc.as_stored(hc.transpose_tiled(x, T), "bf16"), want) is None
    # the first tile untransposed: element (0, 1) of W^T then holds x[0][1] instead of x[1][0] (where the tile has a second column at all)
    if C > 1:
        fails_naming(stored(hc.transpose_tiled(x, T, keep_tile=(0, 0))), want, at=(0, 1))
    # the ragged last tile untransposed
    last = ((R - 1) // T, (C - 1) // T)
    if C > 1:
        fails_naming(stored(hc.transpose_tiled(x, T, keep_tile=last)), want)
    # R and C exchanged in the bound: rows >= C are never written
    fails_naming(stored(hc.transpose_tiled(x, T, swap_bounds=True)), want, at=(0, min(R, C)) if R != C else None)


def test_transpose_cast_shapes():
    assert hc.TRANSPOSE_SHAPES == ((1, 1), (33, 1))


# ------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("case", hc.PATCHIFY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_patchify_cases(case):
    k, Cin, B, H, W, off, route = case
    assert H % k == 0 and W % k == 0
    # the buffers of the GPU file are 16-byte aligned; an offset of one element is 2 (bf16) or 4 (fp32) bytes off
    assert hc.patchify_route(k, Cin, W, out_aligned=off == 0) == route
    for dt in hc.DTYPES:
        img = hc.patchify_image(B, Cin, H, W, dt)
        want = F.unfold(torch.from_numpy(img).float(), kernel_size=k, stride=k).transpose(1, 2).reshape(-1, Cin * k * k)
        assert np.array_equal(hc.as_stored(img, "fp32").astype(np.float64), img)
        ref = hc.patchify_ref(img, k)
        assert np.array_equal(ref, want.double().numpy())
        if dt == "bf16":
            assert np.array_equal(hc.as_stored(ref, "bf16"), want.to(torch.bfloat16).float().numpy()), "P == unfold(img).to(bf16)"
            assert (hc.bf16_round(img) != img).mean() > 0.3, "more than 8 significant bits: the rounding shows"
    routes = [c[-1] for c in hc.PATCHIFY_CASES]
    assert routes.count("strip") >= 2 and routes.count("generic") >= 4
    assert hc.patchify_route(4, 3, 1360) == "strip" and hc.patchify_route(4, 3, 1364) == "generic"
    assert {(c[0], c[1]) for c in hc.PATCHIFY_CASES if c[-1] == "generic"} >= {(2, 8), (8, 1), (4, 4), (4, 3)}


# ------------------------------------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("dt", hc.DTYPES)
def test_rows_cases(dt):
    pc = hc.PIECE[dt]
    for rows, wide in hc.ROWS_CASES:
        C = 520 if wide else pc
        assert C % pc == 0 and (C + 8) % pc == 0
        case = hc.rows_case(rows, C, dt)
        assert np.unique(case.idx).size == rows and case.idx.max() < case.n_log, "rows in idx are unique"
        assert np.unique(case.prow).size == case.n_log
        assert hc.row_trips(rows, C, dt) == 1, "2049 rows of 520 stay within one trip of the grid-stride loop"
        assert case.table.max() < 2 ** 24 and np.array_equal(case.table, np.round(case.table))
        ref = hc.gather_ref(case.table, case)
        hc.as_stored(ref, dt)
        # a gather that ignores the map's offset
        fails_naming(hc.as_stored(hc.gather_ref(case.table, case, use_offset=False), dt), hc.as_stored(ref, dt), at=(0, 0))
        # accumulate: integer data, exact in the output dtype; an accumulate that overwrites
        src = hc.ints(rows, C, mod=113)
        acc = hc.scatter_ref(case.table, src, case, True)
        hc.as_stored(acc, dt)
        first = int(case.prow[case.idx].min())
        msg = fails_naming(hc.as_stored(hc.scatter_ref(case.table, src, case, False), dt), hc.as_stored(acc, dt))
        assert f"first at element ({first}, " in msg
        untouched = np.ones(case.nphys, dtype=bool)
        untouched[case.prow[case.idx]] = False
        assert untouched.any() and np.array_equal(acc[untouched], case.table[untouched])
    rows = hc.ROWS_SECOND_TRIP[dt]
    assert hc.row_trips(rows, 520, dt) == 2 and hc.row_trips(rows - 10, 520, dt) == 1
    big = hc.rows_case(rows, 520, dt)
    assert np.unique(big.idx).size == rows and np.abs(big.table).max() <= 60


# ------------------------------------------------------------------------------------------------ masked_select
def test_masked_select_cases():
    assert all(hc.ms_kernel(n) == "masked_select_kernel" for n in hc.MS_ONE_PASS) and 65536 in hc.MS_ONE_PASS and 0 in hc.MS_ONE_PASS
    assert all(hc.ms_kernel(n) == "masked_select_loop_kernel" for n in hc.MS_LOOP) and 65537 in hc.MS_LOOP
    for n in hc.MS_ONE_PASS + hc.MS_LOOP:
        for pat in hc.MS_PATTERNS:
            lab = hc.ms_labels(n, pat)
            idx = hc.ms_ref(lab, -1)
            assert (np.diff(idx) > 0).all()
            if pat == "none":
                assert idx.size == 0
            elif pat == "all":
                assert idx.size == n
            elif pat == "lane63":
                assert (idx % 64 == 63).all() and idx.size == n // 64
            elif pat == "lane0":
                assert (idx % 64 == 0).all() and idx.size == (n + 63) // 64
            elif pat == "last":
                assert idx.tolist() == ([n - 1] if n else [])
            else:
                assert idx.size == (n - ((n - 1) // 64) * 64 if n else 0) and (n == 0 or idx[-1] == n - 1)
        lab = hc.ms_labels(n, "random", ignore=-100, mixed=True)
        if n > 64:
            assert (lab == -1).any() and (lab == -100).any() and (hc.ms_ref(lab, -100).size > hc.ms_ref(lab, -1).size or True)
            assert (lab[hc.ms_ref(lab, -100)] == -1).any(), "-1 is a real label under ignore_index = -100"


@pytest.mark.parametrize("n", [65, 1025, 65537])
def test_masked_select_dropped_index(n):
    """one selected index lost at a wave boundary: everything behind it moves up by one, the count is one short"""
    lab = hc.ms_labels(n, "all")
    idx = hc.ms_ref(lab, -1)
    want = np.full(n + 1, hc.MS_SENTINEL, dtype=np.int32)
    want[:idx.size] = idx
    got = np.full(n + 1, hc.MS_SENTINEL, dtype=np.int32)
    short = hc.ms_drop_at_wave_boundary(idx)
    got[:short.size] = short
    fails_naming(got, want, at=(64,))


# ------------------------------------------------------------------------------------------------ row_scale, head_grad_prep
@pytest.mark.parametrize("dt", hc.DTYPES)
def test_row_scale_cases(dt):
    for M, rps, C in hc.ROW_SCALE_SHAPES:
        x = hc.values(M, C, dt)
        s = hc.row_scale_factors(M, rps)
        assert set(s) <= set(hc.ROW_SCALE_FACTORS) and s.size == (M + rps - 1) // rps and C % 8 == 0
        ref = hc.row_scale_ref(x, s, rps)
        assert np.array_equal(ref * 2, np.round(ref * 2)) and np.abs(ref).max() < 2 ** 23
        assert np.array_equal(hc.as_stored(ref, dt).astype(np.float64), ref), "exact in the output dtype"
    assert 7 % 3 and 130 % 64, "a ragged last sample"
    assert set(hc.row_scale_factors(130, 64)) | set(hc.row_scale_factors(7, 3)) == set(hc.ROW_SCALE_FACTORS)


def test_head_grad_prep_cases():
    assert hc.head_rstep(48) == (5, 16) and hc.head_rstep(8) == (32, 0) and hc.head_rstep(128) == (2, 0)
    assert any(B < hc.head_rstep(n_pad)[0] for B, n, n_pad in hc.HEAD_SHAPES) and any(B > hc.head_rstep(n_pad)[0] for B, n, n_pad in hc.HEAD_SHAPES)
    for B, n, n_pad in hc.HEAD_SHAPES:
        d = hc.ints(B, n)
        dl, s = hc.head_ref(d, n_pad)
        assert np.array_equal(s, np.round(s)) and np.abs(d).sum(0).max() + hc.HEAD_DB2 < 2 ** 24, "column sums are exact in any order"
        assert (dl[:, n:] == 0).all() and np.array_equal(hc.as_stored(dl, "bf16").astype(np.float64), dl)


# ------------------------------------------------------------------------------------------------ resize
def interpolate(x, src, dst):
    C = x.shape[1]
    t = torch.from_numpy(x).view(1, src[0], src[1], C).permute(0, 3, 1, 2)
    return F.interpolate(t, size=dst, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).reshape(-1, C).numpy()


@pytest.mark.parametrize("src,dst", hc.RESIZE_DYADIC + hc.RESIZE_OTHER, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_cases(src, dst):
    idx, w = hc.resize_terms(src, dst)
    n_src = src[0] * src[1]
    assert idx.min() >= 0 and idx.max() < n_src and np.allclose(w.sum(1), 1.0, atol=1e-6) and (w >= 0).all()
    dyadic = (src, dst) in hc.RESIZE_DYADIC
    assert hc.resize_is_dyadic(idx, w) == dyadic, "every weight of a dyadic case is a multiple of 1/16, and only of a dyadic case"
    for C in hc.RESIZE_C:
        x = hc.resize_input(n_src, C)
        out, bar = hc.resize_fwd_ref(x, idx, w)
        assert np.abs(out - interpolate(x, src, dst)).max() <= 1e-5 * x.max(), "the reference is F.interpolate(mode='bilinear', align_corners=False)"
        g = hc.resize_input(dst[0] * dst[1], C, seed=7)
        adj, abar = hc.resize_adj_ref(g, idx, w, n_src, hc.RESIZE_PREFILL)
        if dyadic:
            assert np.array_equal(out * 16, np.round(out * 16)) and out.max() < 2 ** 12
            assert np.array_equal(adj * 16, np.round(adj * 16)) and adj.max() * 16 < 2 ** 24, "exact in fp32 in any atomic order"
        # <A x, y> == <x, A^T y>
        lhs, rhs = (out * g).sum(), (x * (adj - hc.RESIZE_PREFILL)).sum()
        assert lhs == rhs if dyadic else abs(lhs - rhs) <= 1e-12 * abs(lhs)
    if src == dst:
        assert np.array_equal(idx[:, 0], np.arange(n_src)) and np.array_equal(w[:, 0], np.ones(n_src)), "the identity size is a copy"
    if src == (1, 1):
        assert (w[:, 0] == 1).all(), "a one-pixel source is copied: its clamped neighbours carry no weight"


@pytest.mark.parametrize("src,dst", [((4, 4), (8, 8)), ((4, 4), (1, 8)), ((14, 14), (5, 20))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_unclamped_right_edge(src, dst):
    """x1 not clamped at the right edge: the last target column reads the first pixel of the next row"""
    idx, w = hc.resize_terms(src, dst)
    bad_idx, bad_w = hc.resize_terms(src, dst, clamp_x=False)
    x = hc.resize_input(src[0] * src[1], 3)
    out, bar = hc.resize_fwd_ref(x, idx, w)
    bad, _ = hc.resize_fwd_ref(x, bad_idx, bad_w)
    worst = np.abs(bad - out) / bar
    assert worst.max() > 1e4, "many bars"
    assert int(np.argmax(worst.max(1) > 1)) % dst[1] == dst[1] - 1, "first in the last column"
    if (src, dst) in hc.RESIZE_DYADIC:
        fails_naming(bad.astype(np.float32), out.astype(np.float32), at=(dst[1] - 1, 0))


# ------------------------------------------------------------------------------------------------ the Python side that owns the weight_prep table
def test_prep_table_builder_refuses_what_the_kernel_would_skip():
    """a kind-2 descriptor compiles to nothing in the fp32 instantiation of weight_prep_kernel and the C entry point cannot read a device table: the
    builder of the table (mvlt_amd.params.pack_prep_table, which FlatStore._build_prep goes through) refuses it, with the descriptor's number"""
    from mvlt_amd import params
    from mvlt_amd._lib import MVLTError, PrepDesc
    d = lambda kind, R, C, ld: PrepDesc(256, 512, kind, R, C, ld, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(MVLTError, match="descriptor 1: kind 2"):
        params.pack_prep_table([d(0, 8, 8, 8), d(2, 64, 64, 64)], torch.float32, "cpu")
    with pytest.raises(MVLTError, match="multiples of 8"):
        params.pack_prep_table([d(2, 60, 36, 64)], torch.bfloat16, "cpu")
    with pytest.raises(MVLTError, match="ld_out"):
        params.pack_prep_table([d(0, 9, 8, 8)], torch.float32, "cpu")
    with pytest.raises(MVLTError, match="kind 3"):
        params.pack_prep_table([d(3, 8, 8, 8)], torch.float32, "cpu")
    g = PrepDesc(256, 512, 1, 0, 0, 0, 3, 5, 17, 0, 1, 3, 15, 85, 17, 1)
    tab, blk, n, total, blk_desc = params.pack_prep_table([g, d(0, 65, 63, 70), d(2, 60, 72, 64)], torch.bfloat16, "cpu")
    assert n == 3 and blk.tolist() == [0, 1, 3, 5] and total == 5 and blk_desc.tolist() == [0, 1, 1, 2, 2]
    import ctypes
    assert tab.numel() == 3 * ctypes.sizeof(PrepDesc) and [params.prep_blocks(x) for x in (g, d(0, 65, 63, 70))] == [1, 2]
