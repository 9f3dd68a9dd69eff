"""CPU: the host side of FusedLamb (docs/lamb.md) -- include/mvlt_hip_lamb.h and mvlt_amd/_lib.py LAMB_PROTOTYPES agree and the older tables are as they
were; the tensor and chunk tables built from a CPU store of pvlt_tiny cover every trainable element exactly once, chunk by chunk inside one tensor; the float64
restatement of LAMB that tests/test_lamb_gpu.py measures the kernels against (`lamb_reference` below) gives the hand-computed numbers of a two-tensor case;
and the entry points refuse bad arguments and bad tables without a launch."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from tests.test_host_cpu import _header_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMB = ("mvlt_lamb_version", "mvlt_lamb_check_tables", "mvlt_lamb_moments", "mvlt_lamb_fold", "mvlt_lamb_apply")
LT = dict(mlm=1, itm=1, t2i=1, cls=1)


def lamb_reference(p, g, m, v, layout, table, hp, always_adapt=False, trust_clip=False):
    """THE REFERENCE: LAMB in float64, per tensor, from the values the kernels read (fp32 buffers and fp32 hyper-parameters, promoted).
    p, g, m, v: flat buffers; layout: [(offset, length, group, frozen)]; table: [[lr, weight_decay]] per group; hp: the row of mvlt_adamw_step,
    {-, beta1, beta2, eps, -, 1 - beta1^t, 1 - beta2^t, grad scale} (a clip or gate coefficient already multiplied into the last slot).
    Returns (p, m, v) after the step as float64 buffers -- untouched outside the tensors that train -- and the list of trust ratios (None for frozen ones)."""
    p, g, m, v = (t.detach().double().clone() for t in (p, g, m, v))
    f64 = lambda x: x.detach().double().cpu() if torch.is_tensor(x) else torch.tensor(x, dtype=torch.float64)       # (a Python list: its values as they are)
    _, b1, b2, eps, _, bc1, bc2, gs = f64(hp).tolist()
    table = f64(table).reshape(-1, 2).tolist()
    ratios = []
    for off, n, group, frozen in layout:
        if frozen:
            ratios.append(None)
            continue
        lr, wd = table[group]
        sl = slice(off, off + n)
        gr = g[sl] * gs
        m[sl] = b1 * m[sl] + (1 - b1) * gr
        v[sl] = b2 * v[sl] + (1 - b2) * gr * gr
        u = (m[sl] / bc1) / ((v[sl] / bc2).sqrt() + eps) + wd * p[sl]
        wn, un = float(p[sl].norm()), float(u.norm())
        r = wn / un if (wd != 0 or always_adapt) and wn > 0 and un > 0 else 1.0
        if trust_clip:
            r = min(r, 1.0)
        p[sl] = p[sl] - lr * r * u
        ratios.append(r)
    return p, m, v, ratios


def _lamb_header():
    return open(os.path.join(ROOT, "include", "mvlt_hip_lamb.h")).read()


@pytest.fixture(scope="module")
def tiny():
    """pvlt_tiny with its flat store materialised on the CPU (the store's bookkeeping needs no GPU), one stage and one ragged tensor frozen"""
    from mvlt_amd import pvlt
    m = pvlt.pvlt_tiny(pretrained=False, token_hidden_size=768, num_text_tokens=20, loss_type=LT, pretrained_pth=None, img_size=96)
    m.store.materialize(torch.device("cpu"))
    for n, p in m.named_parameters():
        if n.startswith("block2.") or n == "pos_embed1":
            p.requires_grad_(False)
    return m


# ------------------------------------------------------------------------------------------------------------------ header, binding
def test_lamb_header_and_binding_agree():
    """name by name, parameter by parameter (the rule tests/test_param_groups_cpu.py applies to mvlt_hip_opt.h and OPT_PROTOTYPES)"""
    import mvlt_amd._lib as L
    protos, structs = _header_abi(_lamb_header())
    assert set(protos) == set(L.LAMB_PROTOTYPES) == set(LAMB) and not structs
    older = set(L.PROTOTYPES) | set(L.EXT_PROTOTYPES) | set(L.EMA_PROTOTYPES) | set(L.PLAN_PROTOTYPES) | set(L.OPT_PROTOTYPES)
    assert not set(LAMB) & older                                 # an addition, not an override
    scalars = {"int": C.c_int, "long": C.c_long, "float": C.c_float}
    for name, (ret, params) in protos.items():
        restype, argtypes = L.LAMB_PROTOTYPES[name]
        fn = getattr(L.lib, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name
        assert ret == "int" and restype is C.c_int, name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (ctype, written) in enumerate(zip(argtypes, params)):
            want = scalars[written] if written in scalars else C.c_void_p
            assert written in scalars or written.endswith("*"), (name, i, written)
            assert ctype is want, (name, i, written, ctype)
    assert protos["mvlt_lamb_check_tables"][1] == ["const int64_t*", "int", "const int32_t*", "int", "long", "int"]
    assert protos["mvlt_lamb_moments"][1] == ["const float*", "const float*", "float*", "float*", "long", "const float*", "const int64_t*", "int", "const int32_t*",
                                             "int", "const float*", "int", "float*", "const float*", "const float*", "void*"]
    assert protos["mvlt_lamb_fold"][1] == ["const float*", "int", "const int64_t*", "int", "const float*", "int", "int", "float*", "const float*", "void*"]
    assert protos["mvlt_lamb_apply"][1] == ["float*", "const float*", "const float*", "void*", "long", "const float*", "const int64_t*", "int", "const int32_t*", "int",
                                           "const float*", "int", "const float*", "const float*", "void*"]


def test_lamb_version_and_the_older_tables():
    import mvlt_amd._lib as L
    from mvlt_amd import build, ops
    hdr = _lamb_header()
    assert L.lib.mvlt_lamb_version() == L.LAMB_VERSION == int(re.search(r"#define MVLT_LAMB_VERSION (\d+)", hdr).group(1)) == 1
    assert L.ABI_VERSION == 8 == L.lib.mvlt_abi_version() and L.EXT_VERSION == 1 == L.lib.mvlt_ext_version() and L.EMA_VERSION == 1 == L.lib.mvlt_ema_version()
    assert L.OPT_VERSION == 1 == L.lib.mvlt_opt_version() and L.PLAN_VERSION == 3 == L.lib.mvlt_plan_version()
    assert len(L.PROTOTYPES) == 61 and set(L.EXT_PROTOTYPES) == {"mvlt_ext_version", "mvlt_step_gate", "mvlt_adamw_step_gated"}
    assert set(L.EMA_PROTOTYPES) == {"mvlt_ema_version", "mvlt_ema_update", "mvlt_ema_update_buffers"} and len(L.PLAN_PROTOTYPES) == 14
    assert set(L.OPT_PROTOTYPES) == {"mvlt_opt_version", "mvlt_adamw_step_groups"}
    for name in LAMB:
        assert hasattr(L.lib, name) and name not in L.EXPORTS, name
    assert all(callable(f) for f in (ops.lamb_check_tables, ops.lamb_moments, ops.lamb_fold, ops.lamb_apply))
    for macro, value in (("CHUNK", ops.LAMB_CHUNK), ("ROW", ops.LAMB_ROW), ("ALWAYS_ADAPT", ops.LAMB_ALWAYS_ADAPT), ("TRUST_CLIP", ops.LAMB_TRUST_CLIP)):
        assert int(re.search(rf"#define MVLT_LAMB_{macro} (\d+)", hdr).group(1)) == value, macro
    assert ops.LAMB_CHUNK == 16384 and ops.LAMB_CHUNK % 1024 == 0
    src = open(build.__file__).read()
    assert src.count('"mvlt_hip_lamb.h"') == 2                   # source_hash and _deps_mtime
    assert "lamb.hip" in build._sources()


# ------------------------------------------------------------------------------------------------------------------ the tables
def _coverage(tensors, chunks, total):
    """how often each element of [0, total) is covered by a chunk, with every chunk checked to lie inside its own tensor"""
    from mvlt_amd import ops
    cover = torch.zeros(total, dtype=torch.int32)
    for c, (t, k) in enumerate(chunks.tolist()):
        off, n, _, _, first, cnt = tensors[t].tolist()
        lo, hi = off + k * ops.LAMB_CHUNK, off + min((k + 1) * ops.LAMB_CHUNK, n)
        assert first + k == c and 0 <= k < cnt and off <= lo < hi <= off + n, (c, t, k)            # one tensor, never its neighbour or the gap
        cover[lo:hi] += 1
    return cover


def test_tables_from_a_cpu_store_of_pvlt_tiny(tiny):
    from mvlt_amd import ops
    from mvlt_amd.optim import FusedLamb
    opt = FusedLamb(tiny, lr=1e-3, weight_decay=0.05)
    S = opt._ensure()
    tensors, chunks = opt._tensors, opt._chunks
    assert tensors.dtype == torch.int64 and tuple(tensors.shape) == (len(S.params), ops.LAMB_ROW) and chunks.dtype == torch.int32 and chunks.shape[1] == 2
    assert opt._n_chunks == chunks.shape[0] == int(tensors[:, 5].sum()) and tuple(opt._partials.shape) == (opt._n_chunks, 2)
    cover = _coverage(tensors, chunks, S.total)
    inside = torch.zeros(S.total, dtype=torch.bool)
    group_ix = {id(p): i for i, g in enumerate(opt.param_groups) for p in g["params"]}
    frozen = 0
    for i, (name, p) in enumerate(S.params.items()):
        off, n, _ = S.offsets[name]
        inside[off:off + n] = True
        row = tensors[i].tolist()
        assert row[:4] == [off, n, group_ix[id(p)], 0 if p.requires_grad else 1], name
        assert row[5] == (n + ops.LAMB_CHUNK - 1) // ops.LAMB_CHUNK, name
        frozen += not p.requires_grad
    assert frozen > 20 and int(tensors[:, 3].sum()) == frozen                    # block2.* and pos_embed1
    assert bool((cover[inside] == 1).all())                      # every element of every tensor exactly once (frozen ones too: their flag skips them) ...
    assert int(inside.sum()) < S.total and bool((cover[~inside] == 0).all())     # ... and no alignment gap at all
    big = int(tensors[:, 1].max())
    assert big > 20 * ops.LAMB_CHUNK and int(tensors[:, 5].max()) == (big + ops.LAMB_CHUNK - 1) // ops.LAMB_CHUNK           # the word table: many chunks
    assert int((tensors[:, 1] <= 64).sum()) > 0 and int(tensors[:, 5].min()) == 1                                           # a short tensor: one short chunk
    assert opt.trust_ratios().keys() == S.params.keys() and all(float(r) == 1.0 for r in opt.trust_ratios().values())
    # built once per (store, requires_grad): the same objects until a parameter flips
    first = opt._tensors
    opt._ensure()
    assert opt._tensors is first
    tiny.get_parameter("pos_embed1").requires_grad_(True)
    try:
        opt._ensure()
        i = list(S.params).index("pos_embed1")
        assert opt._tensors is not first and int(opt._tensors[i, 3]) == 0 and int(opt._tensors[:, 3].sum()) == frozen - 1
    finally:
        tiny.get_parameter("pos_embed1").requires_grad_(False)


def test_tables_of_ragged_and_multi_chunk_tensors():
    from mvlt_amd import ops
    from mvlt_amd.optim import lamb_tables
    Ck = ops.LAMB_CHUNK
    lens = [5, 13, 8, 0, Ck - 4, Ck + 8, 3 * Ck + 12, Ck]
    layout, off = [], 0
    for i, n in enumerate(lens):
        layout.append((off, n, i % 3, i == 2))
        off += (n + 7) // 8 * 8
    tensors, chunks = lamb_tables(layout, off, 3)
    assert tensors[:, 5].tolist() == [1, 1, 1, 0, 1, 2, 4, 1] and chunks.shape[0] == 11
    assert chunks.tolist() == [[0, 0], [1, 0], [2, 0], [4, 0], [5, 0], [5, 1], [6, 0], [6, 1], [6, 2], [6, 3], [7, 0]]
    cover = _coverage(tensors, chunks, off)
    inside = torch.zeros(off, dtype=torch.bool)
    for o, n, _, _ in layout:
        inside[o:o + n] = True
    assert bool((cover[inside] == 1).all()) and bool((cover[~inside] == 0).all()) and int((~inside).sum()) == 3 + 3 + 4 + 4
    assert tensors[2].tolist()[2:4] == [2, 1]                    # the frozen flag travels with its row
    # the same tensors in another order: every tensor is cut the same way (chunks count from the tensor's own first element)
    order = [6, 0, 5, 1, 7, 4, 2, 3]
    layout2, off2 = [], 0
    for i in order:
        layout2.append((off2, lens[i], i % 3, i == 2))
        off2 += (lens[i] + 7) // 8 * 8
    t2, _ = lamb_tables(layout2, off2, 3)
    assert [t2[order.index(i), 5].item() for i in range(len(lens))] == tensors[:, 5].tolist()
    empty_t, empty_c = lamb_tables([], 0, 1)
    assert tuple(empty_t.shape) == (0, ops.LAMB_ROW) and tuple(empty_c.shape) == (0, 2)


# ------------------------------------------------------------------------------------------------------------------ the reference itself
def test_reference_on_a_hand_computed_case():
    """beta1 = beta2 = 0.5 at t = 1 from zero moments: m = g / 2, v = g^2 / 2, so m / bc1 = g and sqrt(v / bc2) = |g|; with eps = 0 the Adam part is sign(g).
    Tensor A: p = (6, 8), g = (3, 4), wd = 0.5 -> u = (1 + 3, 1 + 4) = (4, 5), ||p|| = 10, ||u|| = sqrt(41), r = 10 / sqrt(41).
    Tensor B: p = (0), g = (2) -> u = (1), ||p|| = 0 -> r = 1."""
    hp = [0.0, 0.5, 0.5, 0.0, 0.0, 0.5, 0.5, 1.0]
    p = torch.tensor([6.0, 8.0, 99.0, 99.0, 0.0])                # [2:4]: a gap, left alone
    g = torch.tensor([3.0, 4.0, float("nan"), float("nan"), 2.0])
    z = torch.zeros(5)
    layout = [(0, 2, 0, False), (4, 1, 0, False)]
    p2, m2, v2, r = lamb_reference(p, g, z, z, layout, [[0.1, 0.5]], hp)
    assert r == [pytest.approx(10 / math.sqrt(41), rel=1e-15), 1.0]
    assert p2.tolist() == pytest.approx([6 - 0.1 * r[0] * 4, 8 - 0.1 * r[0] * 5, 99.0, 99.0, -0.1], rel=1e-15)
    assert m2.tolist() == [1.5, 2.0, 0.0, 0.0, 1.0] and v2.tolist() == [4.5, 8.0, 0.0, 0.0, 2.0]
    # the gradient factor: gs = 0.5 halves g, the Adam part stays sign(g) -- same u, same r; the moments show it
    hp_half = hp[:7] + [0.5]
    p3, m3, v3, r3 = lamb_reference(p, g, z, z, layout, [[0.1, 0.5]], hp_half)
    assert r3 == r and m3.tolist()[:2] == [0.75, 1.0] and v3.tolist()[:2] == [1.125, 2.0] and p3.tolist() == p2.tolist()
    # trust_clip: r = 10 / sqrt(41) > 1 becomes 1
    p4, _, _, r4 = lamb_reference(p, g, z, z, layout, [[0.1, 0.5]], hp, trust_clip=True)
    assert r4 == [1.0, 1.0] and p4.tolist()[:2] == pytest.approx([6 - 0.4, 8 - 0.5], rel=1e-15)
    # wd = 0: r = 1 (u = sign(g)) unless always_adapt, which gives 10 / sqrt(2)
    p5, _, _, r5 = lamb_reference(p, g, z, z, layout, [[0.1, 0.0]], hp)
    assert r5 == [1.0, 1.0] and p5.tolist()[:2] == pytest.approx([5.9, 7.9], rel=1e-15)
    _, _, _, r6 = lamb_reference(p, g, z, z, layout, [[0.1, 0.0]], hp, always_adapt=True)
    assert r6 == [pytest.approx(10 / math.sqrt(2), rel=1e-15), 1.0]
    # ||u|| = 0: g = m = 0 with wd = 0 (eps > 0 keeps 0 / (0 + eps) = 0) -> r = 1 and p stays, nothing non-finite; a frozen tensor is not touched at all
    hp_eps = hp[:3] + [1e-6] + hp[4:]
    p7, m7, v7, r7 = lamb_reference(p, torch.zeros(5), z, z, [(0, 2, 0, False), (4, 1, 0, True)], [[0.1, 0.0]], hp_eps, always_adapt=True)
    assert r7 == [1.0, None] and p7.tolist() == p.tolist() and not m7.any() and not v7.any()
    # per-group lr / wd: tensor B in a group of its own
    p8, _, _, r8 = lamb_reference(p, g, z, z, [(0, 2, 0, False), (4, 1, 1, False)], [[0.1, 0.5], [0.25, 0.0]], hp)
    assert r8 == r and p8.tolist()[4] == -0.25 and p8.tolist()[:2] == p2.tolist()[:2]


# ------------------------------------------------------------------------------------------------------------------ refusals
def _tables(lens=(5, 13, 16384 + 8)):
    from mvlt_amd.optim import lamb_tables
    layout, off = [], 0
    for i, n in enumerate(lens):
        layout.append((off, n, i % 2, False))
        off += (n + 7) // 8 * 8
    return lamb_tables(layout, off, 2) + (off,)


def test_check_tables_refuses_what_points_outside():
    import mvlt_amd._lib as L
    from mvlt_amd import ops
    tensors, chunks, n = _tables()
    ops.lamb_check_tables(tensors, chunks, n, 2)                 # the tables as built pass
    err = lambda: L.lib.mvlt_last_error()

    def refused(t, c, n_, k, text):
        with pytest.raises(L.MVLTError, match=text):
            ops.lamb_check_tables(t, c, n_, k)
        assert b"mvlt_lamb_check_tables:" in err()

    refused(tensors, chunks, n - 8, 2, "points past n")          # the last tensor ends behind the buffers
    refused(tensors, chunks, n, 1, "names group 1 of 1")

    def edit(row, col, value, which=0):
        t, c = tensors.clone(), chunks.clone()
        (t if which == 0 else c)[row, col] = value
        return t, c

    refused(*edit(2, 1, n), n, 2, "points past n")               # a length that runs off the end
    refused(*edit(1, 0, -8), n, 2, "points past n")
    refused(*edit(1, 0, 10), n, 2, "not a multiple of 4")
    refused(*edit(1, 0, 4), n, 2, "inside or in front of its predecessor")
    refused(*edit(1, 2, 7), n, 2, "names group 7")
    refused(*edit(2, 5, 1), n, 2, "owns chunks")                 # two chunks' worth of elements, one chunk claimed
    refused(*edit(2, 4, 3), n, 2, "owns chunks")
    refused(*edit(3, 1, 0, which=1), n, 2, "chunk 3 is")         # the second chunk of tensor 2 claims to be its first: two workgroups on the same elements
    refused(*edit(3, 0, 1, which=1), n, 2, "chunk 3 is")
    refused(*edit(0, 0, 9, which=1), n, 2, "names tensor 9")
    refused(tensors, chunks[:-1].contiguous(), n, 2, "the chunk table has 3")
    f = L.lib.mvlt_lamb_check_tables
    assert f(None, 3, chunks.data_ptr(), 4, n, 2) < 0 and b"null pointer" in err()
    assert f(tensors.data_ptr(), -1, chunks.data_ptr(), 4, n, 2) < 0 and b"must not be negative" in err()
    assert f(tensors.data_ptr(), 3, chunks.data_ptr(), 4, -8, 2) < 0 and b"must not be negative" in err()
    for k in (0, 255, -1):
        assert f(tensors.data_ptr(), 3, chunks.data_ptr(), 4, n, k) < 0 and b"n_groups" in err(), k
    assert f(None, 0, None, 0, 0, 1) == 0                        # an empty store is fine


def test_launch_refusals_are_error_codes():
    """no launch without a GPU: every call below must come back from the argument checks"""
    import mvlt_amd._lib as L
    lib, err = L.lib, lambda: L.lib.mvlt_last_error()
    a = 4096                                                     # any non-null, aligned address: the checks never dereference
    bad = lambda good, i, v: good[:i] + [v] + good[i + 1:]
    # p, g, m, v, n, hp, tensors, n_tensors, chunks, n_chunks, table, n_groups, partials, gscale_dev, gate, stream
    mom = [a, a, a, a, 64, a, a, 2, a, 2, a, 3, a, None, None, None]
    f = lib.mvlt_lamb_moments
    for i in (0, 1, 2, 3, 5, 6, 8, 10, 12):                      # each required pointer missing in turn
        assert f(*bad(mom, i, None)) < 0 and b"mvlt_lamb_moments: null pointer" in err(), i
    for i in (4, 7, 9):
        assert f(*bad(mom, i, -1)) < 0 and b"must not be negative" in err(), i
    for k in (0, 255, -1):
        assert f(*bad(mom, 11, k)) < 0 and b"n_groups" in err(), k
    assert f(*bad(bad(mom, 13, a), 14, a)) < 0 and b"both gscale_dev and gate" in err()
    for i, v in ((0, a + 8), (1, a + 4), (2, a + 8), (3, a + 12), (6, a + 4), (8, a + 2), (10, a + 4), (12, a + 4)):
        assert f(*bad(mom, i, v)) < 0 and b"aligned" in err(), i
    for i in (4, 7, 9):
        assert f(*bad(mom, i, 0)) == 0                           # nothing to do: no launch
    # partials, n_chunks, tensors, n_tensors, table, n_groups, flags, ratios, gate, stream
    fold = [a, 2, a, 2, a, 3, 0, a, None, None]
    f = lib.mvlt_lamb_fold
    for i in (0, 2, 4, 7):
        assert f(*bad(fold, i, None)) < 0 and b"mvlt_lamb_fold: null pointer" in err(), i
    for i in (1, 3):
        assert f(*bad(fold, i, -1)) < 0 and b"must not be negative" in err(), i
        assert f(*bad(fold, i, 0)) == 0
    assert f(*bad(fold, 5, 255)) < 0 and b"n_groups" in err()
    assert f(*bad(fold, 6, 4)) < 0 and b"unknown flags" in err()
    for i, v in ((0, a + 4), (2, a + 4), (4, a + 4), (7, a + 2)):
        assert f(*bad(fold, i, v)) < 0 and b"aligned" in err(), i
    # p, m, v, p_bf16, n, hp, tensors, n_tensors, chunks, n_chunks, table, n_groups, ratios, gate, stream
    app = [a, a, a, None, 64, a, a, 2, a, 2, a, 3, a, None, None]
    f = lib.mvlt_lamb_apply
    for i in (0, 1, 2, 5, 6, 8, 10, 12):
        assert f(*bad(app, i, None)) < 0 and b"mvlt_lamb_apply: null pointer" in err(), i
    for i in (4, 7, 9):
        assert f(*bad(app, i, -1)) < 0 and b"must not be negative" in err(), i
        assert f(*bad(app, i, 0)) == 0
    assert f(*bad(app, 11, 0)) < 0 and b"n_groups" in err()
    for i, v in ((0, a + 8), (1, a + 4), (2, a + 8), (3, a + 4), (6, a + 4), (8, a + 2), (10, a + 4), (12, a + 2)):
        assert f(*bad(app, i, v)) < 0 and b"aligned" in err(), i


def test_lamb_has_no_cpu_path(tiny):
    from mvlt_amd import ops
    from mvlt_amd._lib import MVLTError
    from mvlt_amd.optim import FusedAdamW, FusedLamb
    tensors, chunks, n = _tables((5, 13))
    z = lambda k=n: torch.zeros(k)
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.lamb_moments(z(), z(), z(), z(), n, z(8), tensors, chunks, z(4), 2, z(4))
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.lamb_fold(z(4), tensors, 2, z(4), 2, 0, z(2))
    with pytest.raises(MVLTError, match="no CPU fallback"):
        ops.lamb_apply(z(), z(), z(), None, n, z(8), tensors, chunks, z(4), 2, z(2))
    opt = FusedLamb(tiny, lr=2e-3, weight_decay=0.05, always_adapt=True)
    assert isinstance(opt, FusedAdamW) and opt.always_adapt and not opt.trust_clip
    assert all(g["eps"] == 1e-6 and g["lr"] == 2e-3 for g in opt.param_groups)           # apex's eps, not AdamW's 1e-8
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05]
    assert FusedLamb(tiny).trust_ratios() == {}                  # no tables before the store was looked at
