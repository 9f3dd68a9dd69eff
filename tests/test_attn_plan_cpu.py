"""CPU: the SR-attention dispatch as a pure function (mvlt_amd/csrc/attn_plan.h through include/mvlt_hip_plan.h): every M against a table written out here, the
launches and chunk counts of the commit BEFORE the plan / launch separation (tests/golden/attn_dispatch.jsonl, its header record says how it was made), the check
path's return codes and error texts, and the LDS budget of every instantiation.  No device is touched."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "attn_dispatch.jsonl")
CSRC = os.path.join(ROOT, "mvlt_amd", "csrc")
BF, F32 = 0, 1


def _fixture():
    lines = [json.loads(x) for x in open(FIXTURE)]
    return lines[0]["header"], [r for r in lines[1:] if "o" in r], [r for r in lines[1:] if "sweep" in r][0]["sweep"]


HEADER, LAUNCHES, SWEEP = _fixture()


def _args(bwd, B, H, N, M, dtype, dkv_dtype=1, **kw):
    """the schedule's contiguous layout, every pointer non-null (the plan never follows one)"""
    import mvlt_amd._lib as L
    Cw = 64 * H
    f = dict(Q=16, KV=32, O=48, lse=64, B=B, H=H, N=N, M=M, ldq=Cw, ldkv=2 * Cw, ldo=Cw, k_off=0, v_off=Cw, scale=0.125, dtype=dtype)
    if bwd:
        f.update(dO=80, dQ=96, dKV=112, lddkv=2 * Cw, dkv_dtype=dkv_dtype)
    f.update(kw)
    return (L.AttnBwdArgs if bwd else L.AttnArgs)(**f)


def _plan(a, streamed=False, want_rc=0):
    import mvlt_amd._lib as L
    p = L.AttnPlan()
    fn = L.lib.mvlt_sr_attention_bwd_plan if isinstance(a, L.AttnBwdArgs) else L.lib.mvlt_sr_attention_fwd_plan
    rc = fn(C.byref(a), int(streamed), C.byref(p))
    assert rc == want_rc, (rc, L.lib.mvlt_last_error())
    if rc:
        return p, None
    buf = C.create_string_buffer(256)
    assert L.lib.mvlt_attn_plan_name(C.byref(p), buf, len(buf)) >= 0
    return p, buf.value.decode()


# ---- (a) the ladders, written out: 32-multiples for NKT; 64 / 128 / 192 / 256 / 288 / 320 for the backward; fwd2 <= 192; resident 320 (bf16) / 288 (fp32).
# An instantiation over the bf16 element type is named as the runtime names it, mangled (the demangler does not know DF16b).
BWD_RUNGS = ((64, (4, 1)), (128, (4, 2)), (192, (4, 3)), (256, (8, 2)), (288, (6, 3)), (320, (8, 3)))


def table_fwd(M, dtype, streamed):
    if streamed or M > (320 if dtype == BF else 288):
        return "_ZN12_GLOBAL__N_122attn_fwd_stream_kernelIDF16bLi128EEEv14mvlt_attn_argsi" if dtype == BF else "attn_fwd_stream_kernel<float, 64>"
    nkt = (M + 31) // 32
    if dtype == BF and M <= 192:
        return f"attn_fwd2_kernel<{nkt}, {'true' if M % 32 != 0 else 'false'}, 4>"
    return f"_ZN12_GLOBAL__N_115attn_fwd_kernelIDF16bLi{nkt}EEEv14mvlt_attn_argsii" if dtype == BF else f"attn_fwd_kernel<float, {nkt}>"


def table_bwd(M, dtype, streamed):
    if streamed or M > (320 if dtype == BF else 288):
        return "_ZN12_GLOBAL__N_122attn_bwd_stream_kernelIDF16bLi4ELi2EEEv18mvlt_attn_bwd_argsii" if dtype == BF else "attn_bwd_stream_kernel<float, 4, 1>"
    nw, tpw = next(inst for top, inst in BWD_RUNGS if M <= top)
    return f"attn_bwd_dma_kernel<{nw}, {tpw}>" if dtype == BF else f"attn_bwd_kernel<float, {nw}, {tpw}>"


def _reachable():
    names = set()
    for M in range(1, 401):
        for dtype in (BF, F32):
            for streamed in (False, True):
                names |= {table_fwd(M, dtype, streamed), table_bwd(M, dtype, streamed)}
    return names


@pytest.mark.parametrize("B,H,N", [(1, 3, 77), (1, 2, 200)])
def test_every_m_plans_the_tabled_kernel(B, H, N):
    bad = []
    for M in range(1, 401):
        for dtype in (BF, F32):
            for streamed in (False, True):
                pf, nf = _plan(_args(False, B, H, N, M, dtype), streamed)
                pb, nb = _plan(_args(True, B, H, N, M, dtype), streamed)
                if (nf, nb) != (table_fwd(M, dtype, streamed), table_bwd(M, dtype, streamed)):
                    bad.append((M, dtype, streamed, nf, nb))
                if nf.startswith("attn_fwd2_kernel"):
                    assert pf.tp[2] == 4 and pf.block == 256 and bool(pf.tp[1]) == (M % 32 != 0)
    assert not bad, bad[:5]
    assert len(_reachable()) == 40                                 # 12 fwd2 + 4 + 9 fwd + 6 bwd_dma + 5 bwd + 2 + 2 streamed


# ---- (b) pinned against the parent commit
def test_fixture_is_what_its_header_says():
    assert re.fullmatch(r"[0-9a-f]{40}", HEADER["parent_commit"]) and len(LAUNCHES) == HEADER["launches"] > 100
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert len({json.dumps(r, sort_keys=True) for r in LAUNCHES}) == len(LAUNCHES)          # distinct records only
    recorded = {HEADER["kernels"][r["o"][0]] for r in LAUNCHES}
    assert recorded == _reachable(), (sorted(_reachable() - recorded), sorted(recorded - _reachable()))


def test_every_recorded_launch_is_planned_exactly():
    """kernel name, grid, block, dynamic LDS bytes, nq_chunks and q_per_wg (the streamed forward's kernel takes nq_chunks alone); which entry point launched a record is
    not recorded, so a resident-range M on a streamed kernel is replanned through the *_streamed form"""
    bad = []
    for r in LAUNCHES:
        k, grid, block, lds, *sc = r["o"]
        name = HEADER["kernels"][k]
        bwd = "bwd" in name
        a = _args(bwd, r["B"], r["H"], r["N"], r["M"], r["dt"], r.get("dkv", 1)) if bwd else _args(False, r["B"], r["H"], r["N"], r["M"], r["dt"])
        streamed = "stream" in name and r["M"] <= (320 if r["dt"] == BF else 288)
        p, got = _plan(a, streamed)
        scal = [p.nq_chunks] if "fwd_stream" in name else [p.nq_chunks, p.q_per_wg]
        if (got, p.grid, p.block, p.lds, scal) != (name, grid, block, lds, sc):
            bad.append((r, name, (got, p.grid, p.block, p.lds, scal)))
    assert not bad, f"{len(bad)} of {len(LAUNCHES)} records differ; first: {bad[:3]}"


def _factor(groups):
    h = max(d for d in range(1, 9) if groups % d == 0)               # the fixture's rule: H = the largest divisor of groups up to 8
    return groups // h, h


def test_chunk_counts_of_the_sweep():
    import mvlt_amd._lib as L
    assert (SWEEP["groups"], SWEEP["N"], SWEEP["M"]) == ([1, 2, 8, 64, 128, 256, 320, 512, 513, 1024],
                                                          [1, 31, 32, 33, 64, 96, 127, 128, 129, 200, 704, 1024, 2432, 4096, 4224, 9216],
                                                          [1, 64, 80, 192, 193, 272, 288, 289, 320, 321, 385])
    bad, seen = [], 0
    for dtype, key in ((BF, "bf16"), (F32, "fp32")):
        for gi, groups in enumerate(SWEEP["groups"]):
            B, H = _factor(groups)
            assert B * H == groups
            for ni, N in enumerate(SWEEP["N"]):
                for mi, M in enumerate(SWEEP["M"]):
                    want = SWEEP[key][gi][ni][mi]
                    p, _ = _plan(_args(True, B, H, N, M, dtype, dkv_dtype=1))
                    got = L.lib.mvlt_sr_attention_bwd_chunks(B, H, N, M, dtype)
                    seen += 1
                    if not (want == got == p.nq_chunks):
                        bad.append((dtype, B, H, N, M, want, got, p.nq_chunks))
    assert seen == 2 * 10 * 16 * 11 and not bad, bad[:5]
    assert any(v > 1 for row in SWEEP["bf16"] for col in row for v in col)
    assert L.lib.mvlt_sr_attention_bwd_chunks(0, 1, 77, 64, 0) == 0 and L.lib.mvlt_sr_attention_bwd_chunks(1, 1, 77, -1, 1) == 0


def test_chunk_count_sets_no_error_text():
    import mvlt_amd._lib as L
    _plan(_args(False, 1, 1, 1, 1, 5), want_rc=-1)
    before = L.lib.mvlt_last_error()
    assert b"bad dtype" in before
    for shape in ((0, 3, 77, 64, 0), (1, 3, 77, 64, 0), (1 << 20, 1 << 12, 9216, 385, 1)):
        L.lib.mvlt_sr_attention_bwd_chunks(*shape)
        assert L.lib.mvlt_last_error() == before


# ---- (c) the check path: same return code and text from the plan and from the launching entry point (which returns before it touches a device).  Texts copied from
# the parent's attention.hip.
STRIDES = "{fn}: strides/offsets must be multiples of {pc} elements"
CHECKS = [
    # (backward?, overrides, streamed forms too?, text)
    (False, dict(Q=None), True, "{fn}: null pointer"),
    (False, dict(O=None), True, "{fn}: null pointer"),
    (True, dict(lse=None), True, "{fn}: null pointer"),
    (True, dict(dKV=None), True, "{fn}: null pointer"),
    (False, dict(N=0), True, "{fn}: bad shape"),
    (False, dict(M=-1), True, "{fn}: bad shape"),
    (True, dict(B=0), True, "{fn}: bad shape"),
    (True, dict(H=-3), True, "{fn}: bad shape"),
    (False, dict(dtype=2), True, "{fn}: bad dtype"),
    (True, dict(dtype=-1), True, "{fn}: bad dtype"),
    (False, dict(dtype=BF, ldq=196), True, STRIDES.format(fn="{fn}", pc=8)),
    (False, dict(dtype=BF, v_off=4), True, STRIDES.format(fn="{fn}", pc=8)),
    (False, dict(dtype=F32, ldkv=386), True, STRIDES.format(fn="{fn}", pc=4)),
    (False, dict(dtype=F32, k_off=2), True, STRIDES.format(fn="{fn}", pc=4)),
    (True, dict(dtype=BF, ldo=196), True, STRIDES.format(fn="{fn}", pc=8)),
    (True, dict(dtype=F32, v_off=194), True, STRIDES.format(fn="{fn}", pc=4)),
    (True, dict(dtype=F32, dkv_dtype=0), True, "{fn}: bf16 dKV needs bf16 operands (it forces one query chunk per (batch, head): plain stores)"),
    (True, dict(dtype=BF, dkv_dtype=0, N=129, M=385), False,
     "mvlt_sr_attention_bwd: a bf16 dKV needs one query chunk per (batch, head); the streamed backward (M=385) takes N <= 128 for it, got N=129"),
]


@pytest.mark.parametrize("bwd,over,streamed_too,text", CHECKS)
def test_check_path_matches_the_entry_point(bwd, over, streamed_too, text):
    import mvlt_amd._lib as L
    base = dict(B=2, H=3, N=77, M=150, dtype=BF)
    base.update(over)
    dkv = base.pop("dkv_dtype", 1)
    a = _args(bwd, base.pop("B"), base.pop("H"), base.pop("N"), base.pop("M"), base.pop("dtype"), dkv, **base) if bwd else \
        _args(False, base.pop("B"), base.pop("H"), base.pop("N"), base.pop("M"), base.pop("dtype"), **base)
    stem = "mvlt_sr_attention_bwd" if bwd else "mvlt_sr_attention_fwd"
    for streamed in ((False, True) if streamed_too else (False,)):
        fn = stem + ("_streamed" if streamed else "")
        want = text.format(fn=fn).encode()
        _plan(a, streamed, want_rc=-1)
        assert L.lib.mvlt_last_error() == want
        assert getattr(L.lib, fn)(C.byref(a), None) == -1 and L.lib.mvlt_last_error() == want


def test_streamed_bf16_dkv_with_several_chunks_is_refused_by_the_streamed_form_too():
    import mvlt_amd._lib as L
    a = _args(True, 2, 3, 129, 150, BF, dkv_dtype=0)
    assert _plan(a, False)[0].nq_chunks == 1                       # resident: a bf16 dKV is GIVEN one chunk
    _plan(a, True, want_rc=-1)
    assert b"takes N <= 128 for it, got N=129" in L.lib.mvlt_last_error()
    assert _plan(_args(True, 2, 3, 128, 150, BF, dkv_dtype=0), True)[0].nq_chunks == 1
    assert L.lib.mvlt_sr_attention_fwd_plan(None, 0, C.byref(L.AttnPlan())) == -1 and L.lib.mvlt_sr_attention_bwd_plan(C.byref(a), 0, None) == -1
    buf = C.create_string_buffer(8)
    assert L.lib.mvlt_attn_plan_name(C.byref(_plan(a)[0]), buf, len(buf)) < 0            # too small a buffer is an error, not a cut name


# ---- (d) LDS budget
def test_lds_of_every_instantiation_fits():
    seen = {}
    for M in range(1, 401):
        for dtype in (BF, F32):
            for streamed in (False, True):
                for bwd in (False, True):
                    p, name = _plan(_args(bwd, 1, 3, 77, M, dtype), streamed)
                    assert seen.setdefault(name, p.lds) == p.lds       # a function of the instantiation alone
    assert set(seen) == _reachable()
    for name, lds in seen.items():
        assert 0 < lds <= (80 if "bwd_stream" in name else 160) * 1024, (name, lds)


# ---- the separation itself
FAMILY_FILES = ("attention_fwd.hip", "attention_fwd2.hip", "attention_bwd.hip", "attention_bwd_dma.hip", "attention_stream.hip")


def test_plan_is_host_only_and_the_launch_side_chooses_nothing():
    plan_h = os.path.join(CSRC, "attn_plan.h")
    text = open(plan_h).read() + open(os.path.join(CSRC, "attention_common.h")).read().split("#ifdef __HIPCC__")[0]
    assert "hip/" not in text and "hipLaunch" not in text and "MVLT_LAUNCH" not in text
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", plan_h], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    launch = open(os.path.join(CSRC, "attention.hip")).read()
    for f in FAMILY_FILES:
        src = open(os.path.join(CSRC, f)).read()
        assert src.count("plan -> launch") == 1 and len(re.findall(r"^int mvlt_launch_attn_\w+\(", src, flags=re.M)) == (2 if f == "attention_stream.hip" else 1)
        launch += src[src.index("plan -> launch"):]
    launch = re.sub(r"//[^\n]*", "", launch)
    for word in ("a.M", "a.N", "a.B", "a->", "<= 192", "320", "288", "512", "1024"):
        assert word not in launch, word
    assert len(open(os.path.join(CSRC, "attention.hip")).read().split("\n")) < 100


def test_case_lists_hold_the_reachable_instantiations_only():
    """the family files' case lists, expanded as their macros expand, against the table of (a)"""
    names = []
    for f in FAMILY_FILES:
        src = open(os.path.join(CSRC, f)).read()
        body = "\n".join(x for x in src[src.index("plan -> launch"):].split("\n") if not x.lstrip().startswith("#") and not x.rstrip().endswith("\\")
                         and "MVLT_ATTN_CASE" not in x)
        body = re.sub(r"//[^\n]*", "", body)
        for mac, argstr in re.findall(r"\b(FWD2|FWD_STREAM|BWD_STREAM|BWD_DMA|FWD|BWD)\(([^()]*)\)", body):
            t = [x.strip() for x in argstr.split(",")]
            if mac == "FWD":
                names.append(table_fwd(32 * int(t[2]), int(t[1]), False))
                assert (t[0] == "bf16") == (t[1] == "0")
            elif mac == "FWD2":
                names += [f"attn_fwd2_kernel<{t[0]}, false, {t[1]}>", f"attn_fwd2_kernel<{t[0]}, true, {t[1]}>"]
            elif mac == "BWD":
                names.append(f"attn_bwd_kernel<float, {t[0]}, {t[1]}>")
            elif mac == "BWD_DMA":
                names.append(f"attn_bwd_dma_kernel<{t[0]}, {t[1]}>")
            elif mac == "FWD_STREAM":
                names.append(table_fwd(400, int(t[1]), True))
            else:
                names.append(table_bwd(400, int(t[1]), True))
    assert len(names) == len(set(names)) == 40 and set(names) == _reachable(), sorted(set(names) ^ _reachable())
