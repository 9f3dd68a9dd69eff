"""CPU: the GEMM dispatch as a pure function (mvlt_amd/csrc/gemm_plan.h through include/mvlt_hip_plan.h), pinned against what the commit BEFORE the
plan / launch separation launched: tests/golden/gemm_dispatch.jsonl holds the distinct GEMM launches of one training step of each bench.py configuration, one
eval forward, the GPU tests that assert kernel names and a set of threshold shapes, recorded on an MI355X from that commit's dispatcher (its header record says how).
No device is touched here."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

from tests.test_host_cpu import _header_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.jsonl")
MAPS = ("a_map", "b_map", "c_map")


TAGS = dict(t="tiny256_b256", m="medium384_b64", f="finetune", e="eval_forward", b="boundary", i="instantiation")


def _fixture():
    """the header, the records in the long form the tests below read (op, the leading dimensions, out = {kernel, grid, block, lds, sc}, tags), the fold launches"""
    lines = [json.loads(x) for x in open(FIXTURE)]
    header, recs = lines[0]["header"], []
    for r in lines[1:-1]:
        o, g = r.pop("o"), r.pop("g", "")
        r["op"] = "nt" if "N" in r else "tn"
        for ld, dim in (("lda", "K"), ("ldb", "K"), ("ldc", "N")) if r["op"] == "nt" else (("lda", "N1"), ("ldb", "N2"), ("ldc", "N2")):
            r.setdefault(ld, r[dim])
        r["out"] = dict(kernel=header["kernels"][o[0]], grid=o[1:4], block=o[4], lds=o[5], sc=o[6:])
        r["tags"] = [TAGS[c] for c in g]
        recs.append(r)
    return header, recs, {tuple(f) for f in lines[-1]["fold"]}


HEADER, RECORDS, FOLDS = _fixture()


def _args(rec):
    """the argument struct of a record: a pointer is -1 (NULL, the default of every pointer but A / B / C) or its low four address bits; every field gets an
    address of its own unless the record says two were the same"""
    import mvlt_amd._lib as L
    cls = L.GemmNTArgs if rec["op"] == "nt" else L.GemmTNArgs
    a = cls()
    for i, (f, t) in enumerate(cls._fields_):
        v = rec.get(f, 0 if f in ("A", "B", "C") else -1) if t is C.c_void_p else rec.get(f, 0)
        if t is C.c_void_p:
            setattr(a, f, None if v < 0 else 0x1000000 * (i + 1) + v)
        elif f in MAPS:
            setattr(a, f, L.RowMap(*rec.get(f, [0] * 11)))
        elif t is not C.c_float:
            setattr(a, f, v)
    if rec.get("R_eq_C"):
        a.R = a.C
    return a


def _plan(a):
    import mvlt_amd._lib as L
    p = L.GemmPlan()
    rc = (L.lib.mvlt_gemm_nt_plan if isinstance(a, L.GemmNTArgs) else L.lib.mvlt_gemm_tn_plan)(C.byref(a), C.byref(p))
    assert rc == 0, L.lib.mvlt_last_error()
    buf = C.create_string_buffer(256)
    assert L.lib.mvlt_gemm_plan_name(C.byref(p), buf, len(buf)) >= 0
    return p, buf.value.decode()


def _scalars(p, kernel):
    """the trailing kernel arguments as the record lists them (a pointer as 0 / 1)"""
    fam = kernel.split("<")[0]
    if fam == "gemm_nt_kernel":
        return [p.nbuf]
    if fam == "gemm_nt_dma_kernel":
        return [p.ns_flags]
    if fam in ("gemm_nt_p8_kernel", "conv3_nt_kernel"):
        return []
    if "gemm_tn_kernel" in fam:
        return [p.per_split]
    return [p.per_split, p.t1, p.t2, p.splits, p.fold]


def _short(rec):
    return {k: v for k, v in rec.items() if k not in ("out", "tags")}


def test_fixture_is_what_its_header_says():
    assert re.fullmatch(r"[0-9a-f]{40}", HEADER["parent_commit"]) and len(RECORDS) == HEADER["records"] and FOLDS
    assert os.path.getsize(FIXTURE) < (1 << 20)
    assert {t for r in RECORDS for t in r["tags"]} == set(TAGS.values())
    assert sum(not r["tags"] for r in RECORDS) > 200              # the records of the tests that assert kernel names
    assert len(set(HEADER["kernels"])) == len(HEADER["kernels"]) == len({r["out"]["kernel"] for r in RECORDS})


def test_every_recorded_launch_is_planned_exactly():
    """kernel name, grid, block, dynamic LDS bytes and scalar arguments of every record; a launch that wrote partial tiles: fold, the scratch bytes, the fold's grid"""
    bad = []
    for rec in RECORDS:
        p, name = _plan(_args(rec))
        out = rec["out"]
        got = dict(kernel=name, grid=list(p.grid), block=p.block, lds=p.lds, sc=_scalars(p, name))
        if got != out:
            bad.append((_short(rec), out, got))
            continue
        wrote_partials = rec["op"] == "tn" and len(out["sc"]) == 5 and out["sc"][4] == 1
        n1, n2 = rec.get("N1"), rec.get("N2")
        if wrote_partials:
            ok = p.fold == 1 and p.partials_need == 2 * p.splits * n1 * n2 and (n1, n2, p.splits, p.fold_grid) in FOLDS
        else:
            ok = p.fold == 0 and p.partials_need == 0 and p.fold_grid == 0
        swapped = name.startswith("gemm_tn_p8_kernel") and name.endswith("true>")
        if not ok or p.swap_operands != swapped:
            bad.append((_short(rec), "fold / swap", (p.fold, p.partials_need, p.fold_grid, p.swap_operands)))
    assert not bad, f"{len(bad)} of {len(RECORDS)} records differ; first: {bad[:3]}"


# ---- every instantiation of the launch switches is pinned

FAMILY_FILES = ("gemm_nt_dma.hip", "gemm_nt_p8.hip", "gemm_tn_dma.hip", "gemm_tn_p8.hip", "gemm_conv3.hip")


def _launch_side(name):
    """a GEMM translation unit from its "plan -> launch" heading to its end"""
    src = open(os.path.join(ROOT, "mvlt_amd", "csrc", name)).read()
    return src[src.index("plan -> launch"):]


def _switch_instantiations():
    """the kernel names behind the case lists of the family files' launch functions, as mvlt_gemm_plan_name prints them"""
    body = "\n".join(_launch_side(f) for f in FAMILY_FILES)
    body = "\n".join(x for x in re.sub(r"\\\n", " ", body).split("\n") if not x.lstrip().startswith("#"))          # the case lists, without the macro definitions
    epis = lambda bn, am: [("NT_DMA", bn, am, e, "64") for e in "12345670"]
    conv = lambda w: [("NT_CONV3", w, bn, e) for bn, es in (("192", "15"), ("64", "125"), ("128", "125")) for e in es]
    modes = lambda bmt, bn, ns: [("TN_DMA", bmt, bn, m, ns, "false") for m in "3012"]
    groups = {"NT_DMA_EPIS": epis, "NT_CONV3_W": conv, "TN_DMA_MODES": modes}
    calls = []
    for mac, argstr in re.findall(r"\b((?:NT|TN)_[A-Z0-9_]+)\(([^()]*)\)", body):
        args = [x.strip() for x in argstr.split(",")]
        calls += groups[mac](*args) if mac in groups else [(mac, *args)]
    fmt = {"NT_F32": lambda bn: f"gemm_nt_kernel<float, {bn}>",
           "NT_DMA": lambda bn, am, epi, bk: f"gemm_nt_dma_kernel<{bn}, {am}, {epi}, {bk}, 128>",
           "NT_P8": lambda *t: f"gemm_nt_p8_kernel<{', '.join(t)}>",
           "NT_CONV3": lambda *t: f"conv3_nt_kernel<{', '.join(t)}>",
           "TN_PLAIN": lambda t, dt, bn: f"gemm_tn_kernel<float, {bn}>" if t == "float" else f"_ZN12_GLOBAL__N_114gemm_tn_kernelIDF16bLi{bn}EEEv17mvlt_gemm_tn_argsi",
           "TN_DMA": lambda *t: f"gemm_tn_dma_kernel<{', '.join(t)}>",
           "TN_P8": lambda *t: f"gemm_tn_p8_kernel<{', '.join(t)}>",
           "TN_CONV3": lambda w: f"conv3_wgrad_kernel<{w}>"}
    return [fmt[c[0]](*c[1:]) for c in calls]


# instantiations that no shape of the three bench configurations and no GPU test of the recorded files reaches, with the reason; the ones a small shape reaches
# have a hand-derived plan in test_hand_derived_plans_of_unrecorded_instantiations
_GENERIC_EPI = "the generic epilogue (EPI 0) on a gathered A: every caller of a gathered NT GEMM has a lean epilogue, except the 2x2 patch gather with row_scale"
_ACT_GATHER = "GELU / GELU' epilogues (EPI 3 / 4) on a gathered A, or on N <= 64: the model's fc1 / fc2 GEMMs read plain rows and are wider"
_SCATTER = "scatter epilogues (EPI 6 / 7: c_map mode 1) on a gathered A: the model scatters only from plain rows"
_STATS_GATHER = "column statistics (EPI 5) behind a patch gather: BatchNorm follows the 3x3 convolutions only"
UNRECORDED = {
    **{f"gemm_nt_dma_kernel<{bn}, {am}, 0, 64, 128>": _GENERIC_EPI for bn, am in ((64, 2), (128, 1), (128, 2))},
    **{f"gemm_nt_dma_kernel<{bn}, {am}, {e}, 64, 128>": _ACT_GATHER for bn in (64, 128) for am in (0, 1, 2) for e in (3, 4) if (bn, am) != (128, 0)},
    **{f"gemm_nt_dma_kernel<{bn}, {am}, {e}, 64, 128>": _SCATTER for bn in (64, 128) for am in (1, 2) for e in (6, 7)},
    **{f"gemm_nt_dma_kernel<{bn}, 1, 5, 64, 128>": _STATS_GATHER for bn in (64, 128)},
    "gemm_nt_dma_kernel<64, 1, 2, 64, 128>": "a residual behind a patch gather with N <= 64: the patch embeddings add none",
    "gemm_nt_dma_kernel<128, 1, 2, 64, 128>": "a residual behind a patch gather: the patch embeddings and the sr convolutions add none",
    "conv3_nt_kernel<16, 192, 1>": "a 192-channel conv3x3 without statistics on a 16-wide map: the decoder's 192-channel convolutions all feed a BatchNorm there",
    "conv3_nt_kernel<64, 128, 1>": "a 64-wide map with 65..128 output channels: the decoder's widest map carries 64 or 192 channels",
    "conv3_nt_kernel<64, 128, 5>": "a 64-wide map with 65..128 output channels: the decoder's widest map carries 64 or 192 channels",
    "gemm_tn_dma_kernel<128, 64, 0, 3, false>": "a 128 x 64 tile with batch-strided rows: the swap in ops.gemm_tn puts the narrow side on N1",
    "gemm_tn_dma_kernel<128, 64, 1, 3, false>": "a 128 x 64 tile behind a patch gather (N2 = r r c_seg <= 64 with N1 > 128): no such convolution in the model",
    "gemm_tn_dma_kernel<128, 64, 2, 3, false>": "a 128 x 64 tile behind a 3x3 gather (N2 = 9 c_seg <= 64): c_seg is a multiple of 8, 9 x 8 = 72",
    "gemm_tn_dma_kernel<64, 128, 0, 3, false>": "a 64 x 128 tile with batch-strided rows: the text-row gradients are wider than 64 on both sides",
    "_ZN12_GLOBAL__N_114gemm_tn_kernelIDF16bLi128EEEv17mvlt_gemm_tn_argsi": "bf16 operands on the register-staged TN kernel need M >= 2^24 rows; the one test that goes there has N2 = 8",
}


def test_every_instantiation_is_recorded_or_listed():
    names = _switch_instantiations()
    assert len(names) == len(set(names)) == 128                   # the file's 130 kernels less the two fold kernels
    recorded = {r["out"]["kernel"] for r in RECORDS}
    assert recorded <= set(names)
    missing = set(names) - recorded
    assert missing == set(UNRECORDED), (sorted(missing - set(UNRECORDED)), sorted(set(UNRECORDED) - missing))


def _nt(M, N, K, **kw):
    return dict(op="nt", M=M, N=N, K=K, lda=kw.pop("lda", K), ldb=K, ldc=N, **kw)


def _tn(M, N1, N2, **kw):
    return dict(op="tn", M=M, N1=N1, N2=N2, lda=kw.pop("lda", N1), ldb=kw.pop("ldb", N2), ldc=N2, **kw)


def _patch(r, w_out, c_seg, h_out=4):
    return [1, 0, 0, 0, r, r * w_out, r * r * w_out * h_out, w_out * h_out, w_out, c_seg, 0]


def _conv3(h, w, c_seg):
    return [2, 0, 0, 0, 3, w, h * w, h * w, w, c_seg, h]


# Derived BY HAND from the parent commit's mvlt_gemm_nt / mvlt_gemm_tn (mvlt_amd/csrc/gemm.hip at the fixture's parent_commit), not from the plan code:
#   128-wide NT kernel: grid = 8 ceil(ceil(M / 128) / 8) ceil(N / bn), bn = 64 for N <= 64 else 128; block 256; ns = min(ceil(K / 64), 2), | 0x100 when there are >= 2 k-steps;
#   LDS = max(ns (128 + bn) 128, 4 32 (bn / 2 + 4) 4) bytes.  EPI: 0 generic (row_scale without R), 2 residual, 3 / 4 GELU / GELU' with bf16 C, 5 column sums,
#   6 / 7 scatter (c_map mode 1) without / with R.
#   conv3x3 NT: grid = 8 ceil(M / 128 / 8) ceil(N / BN); LDS = H_IT 256 16 + 2 BN 128 with H_IT = ceil((128 / W + 2)(W + 2) 8 / 256): W 16 -> 6, W 64 -> 9.
#   128-wide TN kernel, M = 512 (8 k-tiles): chosen splits = min(round8(ceil(512 / tiles)), 8 / 8 = 1) = 1, so m_per_split = 512, grid = t1 t2, LDS = NS 64 (BMT + BN) 2.
#   register-staged TN kernel, M = 2^24: t1 = t2 = 1, splits = min(1024, 262144 k-tiles) = 1024, m_per_split = 256 k-tiles x 64 = 16384, LDS = (128 + 128) 144 + 512.
HAND = [
    (_nt(256, 64, 576, a_map=_conv3(16, 16, 64), row_scale=0, rows_per_scale=256), "gemm_nt_dma_kernel<64, 2, 0, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), row_scale=0, rows_per_scale=256, lda=16), "gemm_nt_dma_kernel<128, 1, 0, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 128, 576, a_map=_conv3(16, 16, 64), row_scale=0, rows_per_scale=256), "gemm_nt_dma_kernel<128, 2, 0, 64, 128>", [8, 1, 1], 256, 65536, [258]),
    (_nt(256, 64, 128, act=1), "gemm_nt_dma_kernel<64, 0, 3, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 64, 128, act=2, H=0), "gemm_nt_dma_kernel<64, 0, 4, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), act=1, lda=16), "gemm_nt_dma_kernel<128, 1, 3, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), act=2, H=0, lda=16), "gemm_nt_dma_kernel<128, 1, 4, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), R=0, lda=16), "gemm_nt_dma_kernel<64, 1, 2, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), R=0, lda=16), "gemm_nt_dma_kernel<128, 1, 2, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), col_sum=0, col_sumsq=0, lda=16), "gemm_nt_dma_kernel<128, 1, 5, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), c_map=_patch(2, 8, 16, 8), lda=16), "gemm_nt_dma_kernel<64, 1, 6, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), c_map=_patch(2, 8, 16, 8), R=0, lda=16), "gemm_nt_dma_kernel<64, 1, 7, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    # (a GELU epilogue or a scatter behind a 3x3 gather is none of the halo kernel's epilogues 1 / 2 / 5 with a plain c_map, and a gather is never BK 32: the 128-wide kernel)
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), act=1, lda=16), "gemm_nt_dma_kernel<64, 1, 3, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), act=2, H=0, lda=16), "gemm_nt_dma_kernel<64, 1, 4, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    (_nt(256, 64, 64, a_map=_patch(2, 8, 16, 8), col_sum=0, col_sumsq=0, lda=16), "gemm_nt_dma_kernel<64, 1, 5, 64, 128>", [8, 1, 1], 256, 24576, [1]),
    (_nt(256, 64, 576, a_map=_conv3(16, 16, 64), act=1), "gemm_nt_dma_kernel<64, 2, 3, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 64, 576, a_map=_conv3(16, 16, 64), act=2, H=0), "gemm_nt_dma_kernel<64, 2, 4, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 128, 576, a_map=_conv3(16, 16, 64), act=1), "gemm_nt_dma_kernel<128, 2, 3, 64, 128>", [8, 1, 1], 256, 65536, [258]),
    (_nt(256, 128, 576, a_map=_conv3(16, 16, 64), act=2, H=0), "gemm_nt_dma_kernel<128, 2, 4, 64, 128>", [8, 1, 1], 256, 65536, [258]),
    (_nt(256, 64, 576, a_map=_conv3(16, 16, 64), c_map=_patch(2, 8, 16, 8)), "gemm_nt_dma_kernel<64, 2, 6, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 64, 576, a_map=_conv3(16, 16, 64), c_map=_patch(2, 8, 16, 8), R=0), "gemm_nt_dma_kernel<64, 2, 7, 64, 128>", [8, 1, 1], 256, 49152, [258]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), c_map=_patch(2, 8, 32, 8), lda=16), "gemm_nt_dma_kernel<128, 1, 6, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 128, 64, a_map=_patch(2, 8, 16, 8), c_map=_patch(2, 8, 32, 8), R=0, lda=16), "gemm_nt_dma_kernel<128, 1, 7, 64, 128>", [8, 1, 1], 256, 34816, [1]),
    (_nt(256, 128, 576, a_map=_conv3(16, 16, 64), c_map=_patch(2, 8, 32, 8)), "gemm_nt_dma_kernel<128, 2, 6, 64, 128>", [8, 1, 1], 256, 65536, [258]),
    (_nt(256, 128, 576, a_map=_conv3(16, 16, 64), c_map=_patch(2, 8, 32, 8), R=0), "gemm_nt_dma_kernel<128, 2, 7, 64, 128>", [8, 1, 1], 256, 65536, [258]),
    (_nt(256, 192, 576, a_map=_conv3(16, 16, 64), lda=64), "conv3_nt_kernel<16, 192, 1>", [8, 1, 1], 256, 6 * 4096 + 2 * 192 * 128, []),
    (_nt(4096, 128, 576, a_map=_conv3(64, 64, 64), lda=64), "conv3_nt_kernel<64, 128, 1>", [32, 1, 1], 256, 9 * 4096 + 2 * 128 * 128, []),
    (_nt(4096, 128, 576, a_map=_conv3(64, 64, 64), lda=64, col_sum=0, col_sumsq=0), "conv3_nt_kernel<64, 128, 5>", [32, 1, 1], 256, 9 * 4096 + 2 * 128 * 128, []),
    (_tn(512, 256, 64, a_map=[0, 64, 128, 0, 0, 0, 0, 0, 0, 0, 0]), "gemm_tn_dma_kernel<128, 64, 0, 3, false>", [2, 1, 1], 256, 3 * 64 * 192 * 2, [512, 2, 1, 1, 0]),
    (_tn(512, 256, 64, b_map=_patch(2, 8, 16, 8), ldb=16), "gemm_tn_dma_kernel<128, 64, 1, 3, false>", [2, 1, 1], 256, 3 * 64 * 192 * 2, [512, 2, 1, 1, 0]),
    (_tn(512, 64, 256, a_map=[0, 64, 128, 0, 0, 0, 0, 0, 0, 0, 0]), "gemm_tn_dma_kernel<64, 128, 0, 3, false>", [2, 1, 1], 256, 3 * 64 * 192 * 2, [512, 1, 2, 1, 0]),
    (_tn(1 << 24, 128, 128), "_ZN12_GLOBAL__N_114gemm_tn_kernelIDF16bLi128EEEv17mvlt_gemm_tn_argsi", [1, 1, 1024], 256, 256 * 144 + 512, [16384]),
]


def test_hand_derived_plans_of_unrecorded_instantiations():
    names = set()
    for rec, kernel, grid, block, lds, sc in HAND:
        p, name = _plan(_args(rec))
        assert (name, list(p.grid), p.block, p.lds, _scalars(p, name)) == (kernel, grid, block, lds, sc), rec
        names.add(kernel)
    # the one instantiation no argument struct reaches: a 3x3 gather has N2 = 9 c_seg >= 72 columns, which is a 128-wide B tile (see its reason in UNRECORDED)
    assert set(UNRECORDED) - names == {"gemm_tn_dma_kernel<128, 64, 2, 3, false>"}
    p, name = _plan(_args(_tn(512, 256, 72, b_map=_conv3(8, 8, 8), ldb=8)))
    assert name == "gemm_tn_dma_kernel<128, 128, 2, 2, false>"


# ---- the measured rules, one shape on each side of every threshold (recorded from the parent under the tag "boundary")

def _field(rec, k):
    """a record's field with the fixture's defaults: pointers other than A / B / C are NULL (-1), everything else 0"""
    import mvlt_amd._lib as L
    types = dict((L.GemmNTArgs if rec["op"] == "nt" else L.GemmTNArgs)._fields_)
    return rec.get(k, -1 if types.get(k) is C.c_void_p and k not in ("A", "B", "C") else 0)


def _boundary_rec(**want):
    hits = [r for r in RECORDS if "boundary" in r.get("tags", []) and all(_field(r, k) == v for k, v in want.items())]
    assert len(hits) == 1, (want, len(hits))
    return hits[0]


def _boundary(**want):
    rec = _boundary_rec(**want)
    return rec["out"]["kernel"], rec["out"]


@pytest.mark.parametrize("below, above, k_below, k_above", [
    # tiles 191 / 192 on the 192 x 256, 256 x 256 and 192 x 320 tiles
    (dict(op="nt", M=36672, N=256), dict(op="nt", M=36864, N=256), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 3, 2, 2, false>"),
    (dict(op="nt", M=48896, N=256), dict(op="nt", M=16384, N=768), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 4, 2, 2, false>"),
    (dict(op="nt", M=36672, N=320, K=128), dict(op="nt", M=36864, N=320, K=128), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 3, 3, 2, false>"),
    # 85 % real work in the whole rounds of padded tiles: ragged 256 x 256 (13920 x 2048 = 84.96 %, 13928 x 2048 = 85.01 % of two rounds) and ragged 192 x 320
    (dict(op="nt", M=13920, N=2048), dict(op="nt", M=13928, N=2048), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 4, 2, 2, true>"),
    (dict(op="nt", M=41776, N=320, K=128), dict(op="nt", M=41784, N=320, K=128), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 3, 3, 2, true>"),
    # ... and at least 384 tiles for the ragged 256 x 256 form: 7944 x 2048 is 97 % of ONE round (256 tiles)
    (dict(op="nt", M=7944, N=2048), dict(op="nt", M=13928, N=2048), "gemm_nt_dma_kernel<128, 0, 1, 64, 128>", "gemm_nt_p8_kernel<1, 4, 2, 2, true>"),
    # BK 32 for EPI 3 / 4 up to K = 512
    (dict(op="nt", M=256, K=512, act=1), dict(op="nt", M=256, K=576, act=1), "gemm_nt_dma_kernel<128, 0, 3, 32, 128>", "gemm_nt_dma_kernel<128, 0, 3, 64, 128>"),
    (dict(op="nt", M=256, K=512, act=2), dict(op="nt", M=256, K=576, act=2), "gemm_nt_dma_kernel<128, 0, 4, 32, 128>", "gemm_nt_dma_kernel<128, 0, 4, 64, 128>"),
    # the 192 x 320 residual epilogue from K = 640 on, whole and ragged
    (dict(op="nt", M=36864, N=320, K=576), dict(op="nt", M=36864, N=320, K=640), "gemm_nt_dma_kernel<128, 0, 2, 64, 128>", "gemm_nt_p8_kernel<2, 3, 3, 2, false>"),
    (dict(op="nt", M=41784, N=320, K=576), dict(op="nt", M=41784, N=320, K=640), "gemm_nt_dma_kernel<128, 0, 2, 64, 128>", "gemm_nt_p8_kernel<2, 3, 3, 2, true>"),
])
def test_nt_thresholds(below, above, k_below, k_above):
    assert _boundary(**below)[0] == k_below and _boundary(**above)[0] == k_above
    for want in (below, above):                                    # ... and the plan agrees (also covered record by record above)
        rec = _boundary_rec(**want)
        assert _plan(_args(rec))[1] == rec["out"]["kernel"]


@pytest.mark.parametrize("M, K, extra, tile", [
    # the smallest whole-tile shapes of the GELU / GELU' epilogues on the 8-phase kernels (tests/test_gelu_p8_gpu.py): 200 tiles of 256 x 256, 192 tiles of 192 x 256
    (6400, 128, {}, "4, 2, 2"), (6400, 192, {}, "4, 2, 2"), (4608, 128, {}, "3, 2, 2"), (4608, 192, {}, "3, 2, 2"), (6144, 128, {}, "3, 2, 2"),
    # ... with a bias, and in the layout of the strided case: lda = ldb = K + 8, ldc = N + 8, batch-strided output rows
    (6400, 128, dict(bias=0), "4, 2, 2"), (4608, 128, dict(bias=0), "3, 2, 2"),
    (6400, 192, dict(lda=200, ldb=200, ldc=2056, c_map=[0, 1280, 1320, 24, 0, 0, 0, 0, 0, 0, 0]), "4, 2, 2"),
    (4608, 192, dict(lda=200, ldb=200, ldc=2056, c_map=[0, 768, 808, 24, 0, 0, 0, 0, 0, 0, 0]), "3, 2, 2"),
])
def test_nt_8_phase_gelu_shapes(M, K, extra, tile):
    """act 1 (with the pre-activation stored) and act 2 at N = 2048: EPI 3 / 4 of the whole-tile 8-phase instantiations, one workgroup per tile in whole XCD groups"""
    for act, epi in ((1, 3), (2, 4)):
        p, name = _plan(_args({**_nt(M, 2048, K, act=act, H=0), **extra}))
        assert name == f"gemm_nt_p8_kernel<{epi}, {tile}, false>", (M, K, act, name)
        bm = 256 if tile[0] == "4" else 192
        assert list(p.grid) == [8 * -(-(M // bm) // 8) * 8, 1, 1] and p.block == 512
    # one k-tile less (K below 128), and one row tile less than 192 tiles of 192 x 256: the 128-wide kernel.  (Below 6400 rows the 256 x 256 tile has fewer than
    # 200 tiles only at 6144 rows, which are one round of 192 x 256 tiles.)
    for act in (1, 2):
        assert _plan(_args({**_nt(M, 2048, 64, act=act, H=0), **extra, "lda": 64, "ldb": 64}))[1].startswith(f"gemm_nt_dma_kernel<128, 0, {2 + act}, ")
        if M == 4608 and "c_map" not in extra:
            assert _plan(_args({**_nt(M - 192, 2048, K, act=act, H=0), **extra}))[1].startswith(f"gemm_nt_dma_kernel<128, 0, {2 + act}, ")


@pytest.mark.parametrize("atomics, partial", [
    # part_min: 7 / 8 m-splits meeting on 128 x 128 outputs
    (dict(M=3584, N1=128, splits=7, partials=0), dict(M=3584, N1=128, splits=8, partials=0)),
    # 16256 / 16384 output elements as recorded (16376 / 16384: test_tn_partial_tiles_from_16384_output_elements)
    (dict(M=3584, N1=127, splits=8, partials=0), dict(M=3584, N1=128, splits=8, partials=0)),
    # TN_MIN_TILES = 8: 63 k-tiles make 7 splits, 64 make 8
    (dict(M=4032, N1=128, N2=128, partials=0, partials_bytes=4 << 20), dict(M=4096, N1=128, N2=128, partials=0, partials_bytes=4 << 20)),
    # partials_bytes one byte short
    (dict(M=4096, N1=128, partials=0, partials_bytes=262143), dict(M=4096, N1=128, partials=0, partials_bytes=262144)),
])
def test_tn_partial_tile_thresholds(atomics, partial):
    for want, wrote in ((atomics, 0), (partial, 1)):
        name, out = _boundary(op="tn", dgrad_out=-1, **want)
        assert name == "gemm_tn_dma_kernel<64, 64, 3, 4, false>" and out["sc"][4] == wrote, (want, out)
        rec = _boundary_rec(op="tn", dgrad_out=-1, **want)
        p, _ = _plan(_args(rec))
        assert p.fold == wrote and (p.partials_need > 0) == bool(wrote)


def test_tn_partial_tiles_from_16384_output_elements():
    """16376 / 16384 elements (N2 % 8 == 0 leaves nothing nearer), derived by hand from the parent's source like HAND: N1 = 2047 | 2048 > 128 and N2 = 8 <= 64 is
    the 128 x 64 tile (NS 3, LDS 3 x 64 x 192 x 2) with t1 = 16, t2 = 1; 8 given splits over 56 k-tiles are 7 k-tiles = 448 rows each, grid 8 x 16; the scratch is
    taken when N1 N2 >= 16384, 8 x 16384 x 2 bytes of it"""
    for n1, wrote in ((2047, 0), (2048, 1)):
        p, name = _plan(_args(_tn(3584, n1, 8, lda=2048, splits=8, partials=0, partials_bytes=4 << 20)))
        assert (name, list(p.grid), p.block, p.lds, _scalars(p, name)) == ("gemm_tn_dma_kernel<128, 64, 3, 3, false>", [128, 1, 1], 256, 73728, [448, 16, 1, 8, wrote])
        assert (p.fold, p.partials_need, p.fold_grid) == ((1, 262144, 64) if wrote else (0, 0, 0))


def test_tn_8_phase_thresholds():
    """the scratch one byte short sends the 256 x 256 and the 192 x 320 tiles to the 128-wide kernel (which then takes partial tiles of its own, fewer splits);
    TN_MIN_TILES on the dgrad kernels: 63 k-tiles = 7 splits, 64 = 8"""
    assert _boundary(op="tn", M=16384, N1=1024, partials_bytes=32 << 20)[0] == "gemm_tn_p8_kernel<4, 2, 2, true, false, false>"
    assert _boundary(op="tn", M=16384, N1=1024, partials_bytes=(32 << 20) - 1)[0] == "gemm_tn_dma_kernel<128, 128, 3, 2, false>"
    assert _boundary(op="tn", M=36864, N1=1280, partials_bytes=26214400)[0] == "gemm_tn_p8_kernel<3, 3, 2, true, true, false>"
    name, out = _boundary(op="tn", M=36864, N1=1280, partials_bytes=26214399)
    assert name == "gemm_tn_dma_kernel<128, 128, 3, 2, false>" and out["sc"][3:] == [16, 1]
    for M, splits in ((4032, 7), (4096, 8)):
        for n in (64, 128):
            name, out = _boundary(op="tn", M=M, N1=n, dgrad_out=0)
            assert name.endswith("true>") and out["sc"][3] == splits


# ---- the ABI addition and the separation itself

def test_plan_header_and_binding_agree():
    """include/mvlt_hip_plan.h against _lib.PLAN_PROTOTYPES / PLAN_STRUCTS, name by name, parameter by parameter, field by field (the rule tests/test_host_cpu.py
    applies to mvlt_hip.h; an array field `int grid[3]` is compared with ctypes' c_int * 3)"""
    import mvlt_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "mvlt_hip_plan.h")).read()
    protos, structs = _header_abi(re.sub(r"(\w+)\[(\d+)\]", r"\1__\2", hdr))
    assert set(protos) == set(L.PLAN_PROTOTYPES) and set(structs) == {n for n, _ in L.PLAN_STRUCTS} == {"mvlt_gemm_plan", "mvlt_attn_plan", "mvlt_mlp_plan"}
    assert not set(L.PLAN_PROTOTYPES) & (set(L.PROTOTYPES) | set(L.EXT_PROTOTYPES) | set(L.EMA_PROTOTYPES))
    classes = dict(L.STRUCTS + L.PLAN_STRUCTS)
    scalars = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "char*": C.c_char_p}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.PLAN_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype is C.c_int and ret == "int" and list(fn.argtypes or []) == list(argtypes), name
        assert len(argtypes) == len(params), name
        for ctype, written in zip(argtypes, params):
            want = scalars[written] if written in scalars else C.POINTER(classes[written[:-1].replace("const", "").strip()])
            assert ctype is want, (name, written, ctype)
    for struct, cls in L.PLAN_STRUCTS:
        fields = structs[struct]
        assert len(fields) == len(cls._fields_)
        for (f, ctype), (written_f, written_t) in zip(cls._fields_, fields):
            base, _, n = written_f.partition("__")
            assert f == base and ctype is ({"int": C.c_int, "long": C.c_long}[written_t] * int(n) if n else {"int": C.c_int, "long": C.c_long}[written_t]), (f, written_f)
    assert L.lib.mvlt_plan_version() == L.PLAN_VERSION == int(re.search(r"#define MVLT_PLAN_VERSION (\d+)", hdr).group(1)) == 3
    assert L.lib.mvlt_gemm_plan_sizeof() == C.sizeof(L.GemmPlan) and L.lib.mvlt_attn_plan_sizeof() == C.sizeof(L.AttnPlan) and L.lib.mvlt_mlp_plan_sizeof() == C.sizeof(L.MlpPlan)
    afams = dict(re.findall(r"#define (MVLT_ATTN_\w+) (\d+)", hdr))
    assert len(afams) == 6 and sorted(map(int, afams.values())) == list(range(1, 7))
    fams = dict(re.findall(r"#define (MVLT_GEMM_\w+) (\d+)", hdr))
    assert len(fams) == 9 and sorted(map(int, fams.values())) == list(range(9))
    assert open(os.path.join(ROOT, "mvlt_amd", "build.py")).read().count('"mvlt_hip_plan.h"') == 2          # the source hash and the rebuild check see the header


def test_plan_is_host_only_and_the_launch_side_chooses_nothing():
    plan_h = os.path.join(ROOT, "mvlt_amd", "csrc", "gemm_plan.h")
    text = open(plan_h).read()
    assert "hip/" not in text and "hipLaunch" not in text and "MVLT_LAUNCH" not in text
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"_kernel<\s*\w+\s*,", code.split("inline int plan_kernel_name")[0])           # the plan names no instantiation
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-x", "c++", plan_h], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    launch = re.sub(r"//[^\n]*", "", "\n".join(_launch_side(f) for f in ("gemm_common.h", "gemm.hip") + FAMILY_FILES))
    for word in ("a.M", "a.K", "a->", "0.85", "16384", "TN_MIN_TILES", "part_min", ">= 192", "% 320", "<= 512", ">= 640"):
        assert word not in launch, word


def test_plan_refuses_what_the_entry_points_refuse_and_plans_nothing_for_no_rows():
    import mvlt_amd._lib as L
    p = L.GemmPlan()
    assert L.lib.mvlt_gemm_nt_plan(C.byref(L.GemmNTArgs()), C.byref(p)) < 0 and b"mvlt_gemm_nt: null operand" in L.lib.mvlt_last_error()
    assert L.lib.mvlt_gemm_tn_plan(C.byref(L.GemmTNArgs()), C.byref(p)) < 0 and b"mvlt_gemm_tn: null operand" in L.lib.mvlt_last_error()
    assert L.lib.mvlt_gemm_nt_plan(None, C.byref(p)) < 0 and L.lib.mvlt_gemm_nt_plan(C.byref(L.GemmNTArgs()), None) < 0
    a = _args(_nt(0, 128, 64))
    p, name = _plan(a)
    assert p.family == 0 and name == "" and list(p.grid) == [0, 0, 0]
    assert L.lib.mvlt_gemm_nt(C.byref(a), None) == 0               # M == 0: no launch, so no device either
    b = _args(_tn(0, 128, 128))
    assert _plan(b)[0].family == 0 and L.lib.mvlt_gemm_tn(C.byref(b), None) == 0
    for bad, text in ((_nt(256, 128, 60), b"multiples of 8"), (_nt(256, 128, 64, act=2), b"needs H"), (_nt(256, 128, 64, post_y=0), b"post_y needs bf16 operands"),
                      (_tn(512, 128, 64, dgrad_out=0, dgrad_wt=0), b"dgrad_out needs"), (_tn(512, 128, 62, ldb=64, c_overwrite=1), b"c_overwrite needs")):
        a = _args(bad)
        plan_fn, run_fn = (L.lib.mvlt_gemm_nt_plan, L.lib.mvlt_gemm_nt) if bad["op"] == "nt" else (L.lib.mvlt_gemm_tn_plan, L.lib.mvlt_gemm_tn)
        assert plan_fn(C.byref(a), C.byref(L.GemmPlan())) == -1 and text in L.lib.mvlt_last_error(), (bad, L.lib.mvlt_last_error())
        assert run_fn(C.byref(a), None) == -1 and text in L.lib.mvlt_last_error()
    buf = C.create_string_buffer(8)
    p, _ = _plan(_args(_nt(256, 128, 64)))
    assert L.lib.mvlt_gemm_plan_name(C.byref(p), buf, len(buf)) < 0          # too small a buffer is an error, not a cut name
