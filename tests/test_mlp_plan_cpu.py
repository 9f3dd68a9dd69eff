"""CPU: the fused-MLP dispatch as a pure function (mvlt_amd/csrc/mlp_plan.h through include/mvlt_hip_plan.h): every shape of a sweep against the rules written out here,
the split arithmetic's invariants, the launches of the commit BEFORE the plan / launch separation (tests/golden/mlp_dispatch.jsonl, its header record says how it was
made), the check path's return codes and error texts, and the LDS bytes of every instantiation.  No device is touched."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mlp_dispatch.jsonl")
CSRC = os.path.join(ROOT, "mvlt_amd", "csrc")
NONE, FUSED, PIPE, WGRAD, WGRAD2 = range(5)
ENTRY = {"fwd": "mvlt_mlp_fwd", "bwd_dx": "mvlt_mlp_bwd_dx", "bwd_dw": "mvlt_mlp_bwd_dw"}
HIDS = (64, 128, 192, 256, 512, 1024)
SCALES = (0, 52, 63, 64, 100, 128, 196)          # 0: no row_scale; else rows_per_scale
MS = range(1, 1101)


def _fixture():
    lines = [json.loads(x) for x in open(FIXTURE)]
    return lines[0]["header"], lines[1:]


HEADER, LAUNCHES = _fixture()


def _args(which, Cdim, hid, M, *, h_out=False, rps=0, **kw):
    """every pointer the entry point needs non-null and 16-byte aligned (the plan never follows one)"""
    import mvlt_amd._lib as L
    f = dict(x=0x100, w1=0x200, b1=0x300, M=M, C=Cdim, hid=hid, row_scale=0x400 if rps else None, rows_per_scale=rps)
    if which == "fwd":
        f.update(wb=0x500, b2=0x600, residual=0x700, out=0x800, h_out=0x900 if h_out else None)
    elif which == "bwd_dx":
        f.update(dy=0xa00, wb=0x500, wc=0xb00, out=0x800, h_out=0x900 if h_out else None)
    else:
        f.update(dy=0xa00, wc=0xb00, dw1=0xc00, db1=0xd00, dw2=0xe00, db2=0xf00)
    f.update(kw)
    return L.MlpArgs(**f)


def _plan(which, a, want_rc=0):
    import mvlt_amd._lib as L
    p = L.MlpPlan()
    rc = getattr(L.lib, ENTRY[which] + "_plan")(C.byref(a), C.byref(p))
    assert rc == want_rc, (rc, L.lib.mvlt_last_error())
    return p


def _name(p):
    import mvlt_amd._lib as L
    buf = C.create_string_buffer(64)
    assert L.lib.mvlt_mlp_plan_name(C.byref(p), buf, len(buf)) >= 0
    return buf.value.decode()


# ---- (a) the rules, written out
def table(which, Cdim, hid, h_out, rps):
    if which == "bwd_dw":
        return f"mlp_wgrad2_kernel<{Cdim}, {4 if Cdim == 64 else 8}>" if rps == 0 or rps % 64 == 0 else f"mlp_wgrad_kernel<{Cdim}>"
    return f"mlp_{'pipe' if not h_out and hid >= 128 else 'fused'}_kernel<{Cdim}, {0 if which == 'fwd' else 1}>"


STAGE = {64: 4 * 16 * 68 * 4, 128: 4 * 16 * 132 * 4}                 # the epilogue's staging: 4 waves x 16 rows x (C + 4) floats


def table_lds(name, Cdim, hid):
    """the parent's launch code, term by term"""
    mode1 = name.endswith(", 1>")
    if name.startswith("mlp_fused"):
        jc = 64 if Cdim == 64 else 32
        return max((2 * jc * Cdim * (2 if mode1 else 1) + 2 * Cdim * jc) * 2 + hid * 4, STAGE[Cdim])
    if name.startswith("mlp_pipe"):
        return max(2 * (2 if mode1 else 1) * 32 * 2 * Cdim + 2 * Cdim * 64 + hid * 4, STAGE[Cdim])
    weights_and_ring = 2 * 128 * Cdim * 2 + 2 * 2 * 64 * 2 * Cdim
    return weights_and_ring + (1664 * 8 if name.startswith("mlp_wgrad2") else 0)


def _reachable():
    return {table(w, Cdim, hid, h, rps) for w in ENTRY for Cdim in (64, 128) for hid in HIDS for h in (False, True) for rps in SCALES
            if not (w == "bwd_dw" and hid % 128)}


def test_exactly_twelve_instantiations_are_reachable():
    assert _reachable() == {f"mlp_{f}_kernel<{c}, {m}>" for f in ("fused", "pipe") for c in (64, 128) for m in (0, 1)} | {
        "mlp_wgrad_kernel<64>", "mlp_wgrad_kernel<128>", "mlp_wgrad2_kernel<64, 4>", "mlp_wgrad2_kernel<128, 8>"}


@pytest.mark.parametrize("Cdim", [64, 128])
@pytest.mark.parametrize("which", ["fwd", "bwd_dx"])
def test_forward_and_input_gradient_plan_the_tabled_kernel(which, Cdim):
    fam = {"mlp_fused": FUSED, "mlp_pipe": PIPE}
    bad, seen = [], set()
    for hid in HIDS:
        for h_out in (False, True):
            for rps in SCALES:
                want = table(which, Cdim, hid, h_out, rps)
                seen.add(_name(_plan(which, _args(which, Cdim, hid, 77, h_out=h_out, rps=rps))))
                for M in MS:
                    p = _plan(which, _args(which, Cdim, hid, M, h_out=h_out, rps=rps))
                    got = (p.family, list(p.tp), p.grid, p.block, p.lds, p.m_per_split, p.splits, p.ny, p.fold, list(p.fold_grid), p.partials_need)
                    if got != (fam[want[:want.index("_kernel")]], [Cdim, which == "bwd_dx"], (M + 127) // 128, 256, table_lds(want, Cdim, hid), 0, 0, 0, 0, [0, 0], 0):
                        bad.append((hid, h_out, rps, M, got))
                assert _name(p) == want
    assert not bad, bad[:5]
    assert seen == {n for n in _reachable() if n.endswith(f"<{Cdim}, {0 if which == 'fwd' else 1}>")}


# ---- (b) the split invariants of the weight-gradient plan, and where the gradients leave to
def fold_wgs(hid, Cdim):
    return (hid * Cdim // 8 + 31) // 32


@pytest.mark.parametrize("Cdim", [64, 128])
def test_weight_gradient_plan_and_its_split_invariants(Cdim):
    bad = []
    for hid in HIDS:
        if hid % 128:
            _plan("bwd_dw", _args("bwd_dw", Cdim, hid, 77), want_rc=-1)
            continue
        for rps in SCALES:
            want = table("bwd_dw", Cdim, hid, False, rps)
            two = want.startswith("mlp_wgrad2")
            for M in MS:
                # partials offered to every launch: exactly what it needs for an even M, one byte less for an odd one
                p0 = _plan("bwd_dw", _args("bwd_dw", Cdim, hid, M, rps=rps))
                need = 2 * p0.splits * hid * Cdim * 2
                p = _plan("bwd_dw", _args("bwd_dw", Cdim, hid, M, rps=rps, partials=0x10000, partials_bytes=need - M % 2))
                ok = (p.family == (WGRAD2 if two else WGRAD) and list(p.tp) == [Cdim, (4 if Cdim == 64 else 8) if two else 0]
                      and p.block == (64 * p.tp[1] if two else 256) and p.lds == table_lds(want, Cdim, hid) and p.ny == hid // 128
                      and p.m_per_split % 64 == 0 and (p.splits - 1) * p.m_per_split < M <= p.splits * p.m_per_split
                      and p.grid == 8 * ((p.splits + 7) // 8) * (hid // 128)
                      and (p.m_per_split, p.splits, p.grid) == (p0.m_per_split, p0.splits, p0.grid) and p0.fold == 0 and list(p0.fold_grid) == [0, 0]
                      and p.fold == int(two and M % 2 == 0) and list(p.fold_grid) == ([fold_wgs(hid, Cdim)] * 2 if p.fold else [0, 0])
                      and p.partials_need == p0.partials_need == (need if two else 0))
                if not ok:
                    bad.append((hid, rps, M, p.family, list(p.tp), p.grid, p.block, p.lds, p.m_per_split, p.splits, p.ny, p.fold, list(p.fold_grid), p.partials_need))
            assert _name(p) == want
    assert not bad, bad[:5]


@pytest.mark.parametrize("over,fold", [
    (dict(), 1),
    (dict(partials=None), 0),
    (dict(partials=0x10008), 0),                  # a scratch that is not 16-byte aligned
    (dict(dw1=0xc04), 0),
    (dict(dw2=0xe08), 0),
    (dict(partials_bytes=-1), 0),                 # one byte short (replaced below)
    (dict(defer_fold=1), 1),
    (dict(row_scale=0x400, rows_per_scale=128), 1),
    (dict(row_scale=0x400, rows_per_scale=100), 0),          # the per-row kernel has atomics only
])
def test_partial_tiles_exactly_where_the_fold_bookkeeping_hands_out_a_region(over, fold):
    Cdim, hid, M = 64, 512, 4241
    need = _plan("bwd_dw", _args("bwd_dw", Cdim, hid, M)).partials_need
    assert need == 2 * 67 * hid * Cdim * 2                 # 67 tiles of 64 rows, a split each
    f = dict(partials=0x10000, partials_bytes=need)
    f.update(over)
    if f["partials_bytes"] == -1:
        f["partials_bytes"] = need - 1
    p = _plan("bwd_dw", _args("bwd_dw", Cdim, hid, M, **f))
    assert p.fold == fold and list(p.fold_grid) == ([fold_wgs(hid, Cdim)] * 2 if fold else [0, 0])


# ---- (c) pinned against the parent commit
def test_fixture_is_what_its_header_says():
    assert re.fullmatch(r"[0-9a-f]{40}", HEADER["parent_commit"]) and len(LAUNCHES) == HEADER["launches"] > 100
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert len({json.dumps(r, sort_keys=True) for r in LAUNCHES}) == len(LAUNCHES)          # distinct records only
    recorded = {HEADER["kernels"][r["o"][0]] for r in LAUNCHES}
    assert recorded == _reachable() and len(recorded) == 12, (sorted(_reachable() - recorded), sorted(recorded - _reachable()))
    assert any(r["pp"] for r in LAUNCHES) and any(r["o"][5] > 1 for r in LAUNCHES if len(r["o"]) > 4)       # partial tiles and several splits were recorded


def test_every_recorded_launch_is_planned_exactly():
    """kernel name, grid, block, dynamic LDS bytes, the three scalar arguments of the weight-gradient kernels, and whether partial-tile pointers were passed"""
    bad = []
    for r in LAUNCHES:
        k, grid, block, lds, *sc = r["o"]
        name = HEADER["kernels"][k]
        which = "bwd_dw" if "wgrad" in name else "fwd" if name.endswith(", 0>") else "bwd_dx"
        kw = dict(rps=r["rps"], row_scale=0x400 if r["rs"] else None)
        if which == "bwd_dw":
            kw.update(dw1=0xc00 + r["al"][0], dw2=0xe00 + r["al"][1], partials=0x10000 + r["al"][2] if r["pt"] else None, partials_bytes=r["pb"])
        else:
            kw.update(h_out=bool(r["h"]))
        p = _plan(which, _args(which, r["C"], r["hid"], r["M"], **kw))
        got = (_name(p), p.grid, p.block, p.lds, [p.m_per_split, p.splits, p.ny] if which == "bwd_dw" else [], p.fold)
        if got != (name, grid, block, lds, sc, r["pp"]):
            bad.append((r, name, got))
    assert not bad, f"{len(bad)} of {len(LAUNCHES)} records differ; first: {bad[:3]}"


# ---- (d) the check path: same return code and text from the plan and from the launching entry point (which returns before it touches a device).  Texts copied from
# the parent's mlp.hip, in its order.
LNB = "mvlt_mlp_bwd_dx: lnb_x needs lnb_mean / lnb_rstd / lnb_gamma / lnb_dx / lnb_partials (and a scale for lnb_dx2), 16-byte aligned"
LN = "mvlt_mlp_fwd: the folded LayerNorm needs gamma, beta, y, mean, rstd and 16-byte aligned rows"
POST = "mvlt_mlp_fwd: post_y needs post_gamma / post_beta / post_mean / post_rstd and 16-byte alignment"
LNB_OK = dict(lnb_x=0x1100, lnb_mean=0x1200, lnb_rstd=0x1300, lnb_gamma=0x1400, lnb_dx=0x1500, lnb_partials=0x1600)
CHECKS = [
    ("fwd", dict(x=None), "mvlt_mlp_fwd: null pointer"),
    ("fwd", dict(w1=None), "mvlt_mlp_fwd: null pointer"),
    ("fwd", dict(out=None), "mvlt_mlp_fwd: null pointer"),
    ("bwd_dx", dict(wb=None), "mvlt_mlp_bwd_dx: null pointer"),
    ("bwd_dx", dict(b1=None), "mvlt_mlp_bwd_dx: null pointer"),
    ("fwd", dict(C=96), "mvlt_mlp_fwd: C must be 64 or 128 (stage 1 / 2), got 96"),
    ("bwd_dx", dict(C=96), "mvlt_mlp_bwd_dx: C must be 64 or 128 (stage 1 / 2), got 96"),
    ("fwd", dict(hid=96), "mvlt_mlp_fwd: hidden size must be a multiple of 64"),
    ("bwd_dx", dict(hid=0), "mvlt_mlp_bwd_dx: hidden size must be a multiple of 64"),
    ("fwd", dict(row_scale=0x400), "mvlt_mlp_fwd: row_scale needs rows_per_scale"),
    ("bwd_dx", dict(row_scale=0x400, rows_per_scale=-1), "mvlt_mlp_bwd_dx: row_scale needs rows_per_scale"),
    ("fwd", dict(b2=None), "mvlt_mlp_fwd: b2 and residual are required"),
    ("fwd", dict(residual=None), "mvlt_mlp_fwd: b2 and residual are required"),
    ("fwd", dict(out_op=0x2008), "mvlt_mlp_fwd: out_op must be 16-byte aligned"),
    ("fwd", dict(post_y=0x2100), POST),
    ("fwd", dict(post_y=0x2108, post_gamma=1, post_beta=2, post_mean=3, post_rstd=4), POST),
    ("fwd", dict(ln_x=0x2200), LN),
    ("fwd", dict(ln_x=0x2200, ln_gamma=1, ln_beta=2, ln_mean=3, ln_rstd=4), LN),                       # no ln_y
    ("fwd", dict(ln_x=0x2204, ln_gamma=1, ln_beta=2, ln_mean=3, ln_rstd=4, ln_y=0x2300), LN),
    ("bwd_dx", dict(dy=None), "mvlt_mlp_bwd_dx: dy and wc (W2^T) are required"),
    ("bwd_dx", dict(wc=None), "mvlt_mlp_bwd_dx: dy and wc (W2^T) are required"),
    ("bwd_dx", dict(LNB_OK, lnb_partials=None), LNB),
    ("bwd_dx", dict(LNB_OK, lnb_mean=None), LNB),
    ("bwd_dx", dict(LNB_OK, lnb_dx2=0x1700), LNB),                                                    # no scale
    ("bwd_dx", dict(LNB_OK, lnb_dx2=0x1700, lnb_dx2_scale=0x1800), LNB),                              # no rows per scale
    ("bwd_dx", dict(LNB_OK, lnb_dx=0x1508), LNB),
    ("bwd_dw", dict(dw2=None), "mvlt_mlp_bwd_dw: null pointer"),
    ("bwd_dw", dict(x=None), "mvlt_mlp_bwd_dw: null pointer"),
    ("bwd_dw", dict(C=96), "mvlt_mlp_bwd_dw: C must be 64 or 128, got 96"),
    ("bwd_dw", dict(hid=64), "mvlt_mlp_bwd_dw: hidden size must be a multiple of 128"),
    ("bwd_dw", dict(hid=96), "mvlt_mlp_bwd_dw: hidden size must be a multiple of 128"),
    ("bwd_dw", dict(row_scale=0x400), "mvlt_mlp_bwd_dw: row_scale needs rows_per_scale"),
    # the one addition: a size the runtime could only refuse at the launch
    ("bwd_dx", dict(hid=34880), "mvlt_mlp_bwd_dx: hid=34880 needs 164096 B of LDS (>160 KB)"),
    ("fwd", dict(hid=32832, h_out=0x900), "mvlt_mlp_fwd: hid=32832 needs 164096 B of LDS (>160 KB)"),
]


@pytest.mark.parametrize("which,over,text", CHECKS)
@pytest.mark.parametrize("M", [77, 0])
def test_check_path_matches_the_entry_point(which, over, text, M):
    """M = 0: the checks come first, the empty launch behind them"""
    import mvlt_amd._lib as L
    over = dict(over)
    a = _args(which, 64, over.pop("hid", 256), M, **over)
    if "needs 164096 B" in text and M == 0:                 # a bound on the choice, which an empty launch does not make
        assert _plan(which, a).family == NONE
        return
    _plan(which, a, want_rc=-1)
    assert L.lib.mvlt_last_error() == text.encode()
    assert getattr(L.lib, ENTRY[which])(C.byref(a), None) == -1 and L.lib.mvlt_last_error() == text.encode()


@pytest.mark.parametrize("which", list(ENTRY))
def test_an_empty_launch_is_planned_as_none_behind_the_checks(which):
    import mvlt_amd._lib as L
    for M in (0, -5):
        a = _args(which, 128, 256, M, **(LNB_OK if which == "bwd_dx" else {}))
        p = _plan(which, a)
        assert p.family == NONE and _name(p) == "" and (p.grid, p.block, p.lds, p.splits, p.fold) == (0, 0, 0, 0, 0)
        assert getattr(L.lib, ENTRY[which])(C.byref(a), None) == 0                 # nothing is launched: no device is touched
    fn = getattr(L.lib, ENTRY[which] + "_plan")
    assert fn(None, C.byref(L.MlpPlan())) == -1 and fn(C.byref(a), None) == -1
    assert getattr(L.lib, ENTRY[which])(None, None) == -1 and L.lib.mvlt_last_error() == (ENTRY[which] + ": null pointer").encode()
    buf = C.create_string_buffer(8)
    assert L.lib.mvlt_mlp_plan_name(C.byref(_plan(which, _args(which, 64, 256, 77))), buf, len(buf)) < 0       # too small a buffer is an error, not a cut name
    unknown = L.MlpPlan(family=9)
    assert L.lib.mvlt_mlp_plan_name(C.byref(unknown), C.create_string_buffer(64), 64) < 0


# ---- (e) LDS
PARENT_LDS = {           # the numbers the parent's launch functions compute at hid = 128 and 512 (the weight-gradient kernels' do not depend on hid)
    "mlp_fused_kernel<64, 0>": (33280, 34816), "mlp_fused_kernel<64, 1>": (49664, 51200),
    "mlp_fused_kernel<128, 0>": (33792, 34816), "mlp_fused_kernel<128, 1>": (49664, 51200),
    "mlp_pipe_kernel<64, 0>": (17408, 18432), "mlp_pipe_kernel<64, 1>": (25088, 26624),
    "mlp_pipe_kernel<128, 0>": (33792, 34816), "mlp_pipe_kernel<128, 1>": (49664, 51200),
    "mlp_wgrad_kernel<64>": (65536, 65536), "mlp_wgrad_kernel<128>": (131072, 131072),
    "mlp_wgrad2_kernel<64, 4>": (78848, 78848), "mlp_wgrad2_kernel<128, 8>": (144384, 144384),
}


def _plans_at(hid):
    out = {}
    for Cdim in (64, 128):
        for which in ("fwd", "bwd_dx"):
            for h_out in (False, True):
                p = _plan(which, _args(which, Cdim, hid, 300, h_out=h_out))
                out[_name(p)] = p.lds
        for rps in (0, 100):
            p = _plan("bwd_dw", _args("bwd_dw", Cdim, hid, 300, rps=rps))
            out[_name(p)] = p.lds
    return out


def test_lds_of_every_instantiation():
    assert set(PARENT_LDS) == _reachable()
    at128, at512, at1024 = _plans_at(128), _plans_at(512), _plans_at(1024)            # 1024: the largest hidden size of the BASELINE configurations (C = 128, ratio 8)
    assert set(at128) == set(at512) == set(at1024) == set(PARENT_LDS)
    for name, (a, b) in PARENT_LDS.items():
        assert (at128[name], at512[name]) == (a, b), name
        assert 0 < at1024[name] <= 160 * 1024, (name, at1024[name])
        assert at1024[name] == table_lds(name, int(re.search(r"<(\d+)", name).group(1)), 1024)


# ---- the separation itself
FAMILY_FILES = ("mlp_fused.hip", "mlp_pipe.hip", "mlp_wgrad.hip")


def test_plan_is_host_only_and_the_launch_side_chooses_nothing():
    plan_h = os.path.join(CSRC, "mlp_plan.h")
    text = open(plan_h).read() + open(os.path.join(CSRC, "mlp_common.h")).read().split("#ifdef __HIPCC__")[0]
    assert "hip/" not in text and "hipLaunch" not in text and "MVLT_LAUNCH" not in text
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", plan_h], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    launch = open(os.path.join(CSRC, "mlp.hip")).read()
    for f in FAMILY_FILES:
        src = open(os.path.join(CSRC, f)).read()
        assert src.count("plan -> launch") == 1 and len(re.findall(r"^int mvlt_launch_mlp_\w+\(", src, flags=re.M)) == 1
        launch += src[src.index("plan -> launch"):]
    launch = re.sub(r"//[^\n]*", "", launch)
    for word in ("a.M", "a->", "h_out", "rows_per_scale", "row_scale", ">= 128", "% 64", "splits +", "/ 64"):
        assert word not in launch, word
    # the rules are stated once in the sources, in the plan
    for f in sorted(os.listdir(CSRC)):
        if f != "mlp_plan.h" and f.startswith("mlp"):
            src = open(os.path.join(CSRC, f)).read()
            assert "hid >= 128" not in src and "% 64 == 0" not in src, f
    from mvlt_amd import build
    for f in FAMILY_FILES:
        assert build.EXTRA[f] == ["-fno-slp-vectorize"]               # or the pipelined kernels' ISA changes
    for macro in ("MVLT_GELU_LUT ", "MVLT_GELU_LUT)", "MVLT_PIPE_WAVES_64_1"):
        assert not any(macro in open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))), macro


def test_case_lists_hold_the_reachable_instantiations_only():
    names = []
    for f in FAMILY_FILES:
        src = open(os.path.join(CSRC, f)).read()
        body = "\n".join(x for x in src[src.index("plan -> launch"):].split("\n") if not x.lstrip().startswith("#"))
        body = re.sub(r"//[^\n]*", "", body)
        for mac, argstr in re.findall(r"\b(FUSED|PIPE|WGRAD2|WGRAD)\(([^()]*)\)", body):
            t = [x.strip() for x in argstr.split(",")]
            names.append({"FUSED": "mlp_fused_kernel<{}, {}>", "PIPE": "mlp_pipe_kernel<{}, {}>", "WGRAD": "mlp_wgrad_kernel<{}>", "WGRAD2": "mlp_wgrad2_kernel<{}, {}>"}[mac].format(*t))
    assert len(names) == len(set(names)) == 12 and set(names) == _reachable(), sorted(set(names) ^ _reachable())
