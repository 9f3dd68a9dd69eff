"""GPU: the SR-attention kernels (csrc/attention_<family>.hip, dispatched by csrc/attn_plan.h) on inputs that make single keys decisive, at both sides of every rung of every
dispatch ladder, through strided layouts with guards, and at the numeric edges -- against the float64 reference of tests/attn_cases.py
(softmax(Q K^T scale) V and its autograd from the operands as the kernel reads them).  The inputs' premises are pinned on the CPU by
tests/test_attention_cases_cpu.py.

Bars (the project's parity bars, per element / per (batch, head) slice instead of against one global maximum):
  O     |err| <= TOL x max|V|            TOL 2e-2 (bf16) / 1e-3 (fp32); max|V| = 3 on the decisive inputs
  lse   |err| <= LSE_TOL x max(1, |ref|) LSE_TOL 2e-2 / 1e-3
  dQ, dK, dV (each on its own)  max|err| over a (batch, head) slice <= GRAD_TOL x max|ref| over that slice, GRAD_TOL 3e-2 / 2e-3
A failure prints batch, head, query, the key the query selects and the key whose V row the output is nearest to.

EVERY launch of this file goes through `run()`: operands and results live in flat buffers filled with the sentinel 7.0, with the row
gaps of the layout, one guard row behind O, dQ and dKV and one guard element behind lse; after the launch every sentinel must be
bit-identical (integer view).  Idle workgroups (B H not a multiple of 8) and partial 32-query tiles write nothing they do not own.

Instantiation -> the case that launches it and asserts its name (mvlt_amd._lib.last_kernel(); test_every_instantiation at
(B, H, N) = (1, 3, 77), test_backward_across_query_chunks at (1, 2, 200); NKT = ceil(M / 32)):
  attn_fwd2_kernel<NKT, PADDED, 4>  bf16 public forward, M <= 192
      <1,true> M 1, 31   <1,false> 32   <2,true> 33   <2,false> 64   <3,true> 65   <3,false> 96   <4,true> 97   <4,false> 128
      <5,true> 129       <5,false> 160  <6,true> 161  <6,false> 192
  attn_fwd_kernel<bf16, NKT>        bf16 public forward, 193 <= M <= 320
      <7> 193, 224   <8> 225, 256   <9> 257, 288   <10> 289, 320          (NKT <= 6 is not instantiated in bf16: attn_fwd2_kernel takes it)
  attn_fwd_kernel<float, NKT>       fp32 public forward, M <= 288
      <1> 1, 31, 32   <2> 33, 64   <3> 65, 96   <4> 97, 128   <5> 129, 160   <6> 161, 192   <7> 193, 224   <8> 225, 256   <9> 257, 288
      (<float, 10> is not instantiated: fp32 M > 288 streams)
  attn_bwd_dma_kernel<NW, TPW>      bf16 public backward, M <= 320
      <4,1> 1..64   <4,2> 65..128   <4,3> 129..192   <8,2> 193..256   <6,3> 257, 288   <8,3> 289, 320
  attn_bwd_kernel<float, NW, TPW>   fp32 public backward, M <= 288
      <4,1> 1..64   <4,2> 65..128   <4,3> 129..192   <8,2> 193..256   <6,3> 257, 288      (<float, 8, 3> is not instantiated: fp32 M > 288 streams)
  attn_fwd_stream_kernel<bf16, 128> / attn_bwd_stream_kernel<bf16, 4, 2>     bf16 public M 321, 385; the *_streamed exports at every M
  attn_fwd_stream_kernel<float, 64> / attn_bwd_stream_kernel<float, 4, 1>    fp32 public M 289, 320, 321, 385; the *_streamed exports at every M
The tables below (expected_fwd, expected_bwd, bwd_ladder) are the independent statement of the ladders; run() also asks the library's own plan
(ops.attention_plan, no launch) and holds it to the kernel that ran.  tests/test_attn_plan_cpu.py checks the plan at every M without a GPU.
"""
import math
import re
import types

import pytest
import torch

from tests import attn_cases as ac

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DT_ID = {BF: "bf16", F32: "fp32"}
TOL = {F32: 1e-3, BF: 2e-2}
LSE_TOL = {F32: 1e-3, BF: 2e-2}
GRAD_TOL = {F32: 2e-3, BF: 3e-2}
SENTINEL = 7.0
INT_VIEW = {BF: torch.int16, F32: torch.int32}
HD = ac.HD


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


# ------------------------------------------------------------------------------------------------ which kernel a launch must reach
def resident(M, dtype):
    return M <= (320 if dtype == BF else 288)


def bwd_ladder(M):
    for top, inst in ((64, (4, 1)), (128, (4, 2)), (192, (4, 3)), (256, (8, 2)), (288, (6, 3)), (320, (8, 3))):
        if M <= top:
            return inst
    raise AssertionError(M)


def expected_fwd(M, dtype, streamed):
    if streamed or not resident(M, dtype):
        return "attn_fwd_stream_kernel", (dtype, 128 if dtype == BF else 64)
    nkt = (M + 31) // 32
    if dtype == BF and M <= 192:
        return "attn_fwd2_kernel", (nkt, M % 32 != 0, 4)
    return "attn_fwd_kernel", (dtype, nkt)


def expected_bwd(M, dtype, streamed):
    if streamed or not resident(M, dtype):
        return "attn_bwd_stream_kernel", (dtype, 4, 2 if dtype == BF else 1)
    return ("attn_bwd_dma_kernel", bwd_ladder(M)) if dtype == BF else ("attn_bwd_kernel", (dtype,) + bwd_ladder(M))


def ran(expected):
    """the kernel launched last on this thread must be the instantiation `expected` = (name, template arguments).  Instantiations over the bf16
    element type come back mangled (the C++ runtime's demangler does not know that type): the template arguments are looked up in the mangled form then."""
    base, targs = expected
    name = last_kernel()
    if name.startswith("_Z"):
        enc = lambda t: "DF16b" if t is BF else "f" if t is F32 else f"Lb{int(t)}E" if isinstance(t, bool) else f"Li{t}E"
        want = f"{len(base)}{base}I" + "".join(enc(t) for t in targs) + "E"
        assert want in name, f"meant to reach {base}{targs} ({want}), the library launched {name}"
    else:
        txt = lambda t: "__bf16" if t is BF else "float" if t is F32 else str(t).lower() if isinstance(t, bool) else str(t)
        want = f"{base}<" + ", ".join(txt(t) for t in targs) + ">"
        assert name == want, f"meant to reach {want}, the library launched {name}"


def planned(plan):
    """the instantiation a plan names (ops.attention_plan(...).name: demangled text, or the mangled name of an instantiation over bf16) as ran() takes it"""
    name = plan.name
    if name.startswith("_Z"):
        base, enc = re.fullmatch(r"_ZN12_GLOBAL__N_1\d+([a-z_0-9]+?)I(.*)EEv\d+mvlt_\w+", name).groups()
        targs = tuple(BF if t == "DF16b" else F32 if t == "f" else bool(int(t[2:-1])) if t[1] == "b" else int(t[2:-1]) for t in re.findall(r"DF16b|f|L[ib]\d+E", enc))
    else:
        base, txt = re.fullmatch(r"(\w+)<(.*)>", name).groups()
        targs = tuple(F32 if t == "float" else t == "true" if t in ("true", "false") else int(t) for t in txt.split(", "))
    return base, targs


# ------------------------------------------------------------------------------------------------ layouts, buffers, guards
def contiguous(C):
    """the schedule's layout"""
    return types.SimpleNamespace(ldq=C, ldkv=2 * C, ldo=C, lddkv=2 * C, k_off=0, v_off=C, q_col0=0)


def strided(C):
    """Q (and dQ) a column window of a wider buffer, K and V at offsets inside padded kv rows, padded O / dO rows; dKV rows of 2C + 8 with the
    same offsets: a dV row ends in the first 8 (dead) columns of the next row.  Legal for both dtypes (multiples of 8 elements)."""
    return types.SimpleNamespace(ldq=C + 64, ldkv=2 * C + 32, ldo=C + 8, lddkv=2 * C + 8, k_off=8, v_off=C + 16, q_col0=64)


def live_index(B, R, ld, offs, W, base=0):
    """flat positions of the live elements of a [B, R, len(offs) * W] tensor stored with row stride `ld`, its column blocks at `offs`"""
    rows = torch.arange(B * R).reshape(B, R, 1) * ld
    cols = torch.cat([o + torch.arange(W) for o in offs]).reshape(1, 1, -1)
    return base + rows + cols


class Buf:
    """a flat device buffer of sentinels with the live elements of one tensor inside it and `guard` sentinels behind the last live one"""

    def __init__(self, idx, dtype, guard, dense=None, live=0.0):
        flat = idx.reshape(-1)
        assert flat.unique().numel() == flat.numel(), "the layout overlaps itself"
        size = (int(flat.max()) + 1 + 7) // 8 * 8 + guard
        host = torch.full((size,), SENTINEL, dtype=dtype)
        host[flat] = dense.reshape(-1).to(dtype) if dense is not None else torch.full((flat.numel(),), live, dtype=dtype)
        self.idx, self.dtype, self.t = idx, dtype, host.to(dev())
        self.dead = torch.ones(size, dtype=torch.bool)
        self.dead[flat] = False

    def dense(self):
        return self.t.cpu()[self.idx]

    def check_sentinels(self, what):
        got = self.t.cpu().view(INT_VIEW[self.dtype])[self.dead]
        want = torch.tensor([SENTINEL], dtype=self.dtype).view(INT_VIEW[self.dtype])
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} sentinels overwritten; first at flat element "
                                  f"{int(self.dead.nonzero()[bad[0, 0], 0])} of {self.dead.numel()}; last kernel {last_kernel()}")


def run(ops, case, streamed=False, layout=None, forward=True, backward=True, dkv_fill=0.0, own=False):
    """forward and backward of `case` through the public entry points or the *_streamed exports, in `layout`, with guards; -> namespace of dense
    float64 CPU results (o, lse, dq, dk, dv).  The backward reads the operands O and lse the reference hands it (case.ref, rounded to their dtypes), so
    that it is judged on its own; own=True: the forward's O and lse, as the schedule composes the two."""
    B, H, N, M, C, dt = case.B, case.H, case.N, case.M, case.C, case.dtype
    L = layout or contiguous(C)
    iq = live_index(B, N, L.ldq, [0], C, base=L.q_col0)
    io = live_index(B, N, L.ldo, [0], C)
    ikv = live_index(B, M, L.ldkv, [L.k_off, L.v_off], C)
    idkv = live_index(B, M, L.lddkv, [L.k_off, L.v_off], C)
    ilse = torch.arange(B * H * N).reshape(B, H, N)
    q, kv = Buf(iq, dt, 0, case.q), Buf(ikv, dt, 0, case.kv)
    out = types.SimpleNamespace()
    what = f"{DT_ID[dt]} B{B} H{H} N{N} M{M} {'streamed export' if streamed else 'public'}"
    o = lse = None
    if forward:
        o, lse = Buf(io, dt, L.ldo), Buf(ilse, F32, 1)
        fwd_args = (q.t[L.q_col0:], kv.t, o.t, lse.t, B, H, N, M, L.ldq, L.ldkv, L.ldo, L.k_off, L.v_off, case.scale)
        (ops.sr_attention_fwd_streamed if streamed else ops.sr_attention_fwd)(*fwd_args)
        ran(expected_fwd(M, dt, streamed))
        ran(planned(ops.attention_plan(*fwd_args, streamed=streamed)))
        torch.cuda.synchronize()
        for b, n in ((o, "O"), (lse, "lse"), (q, "Q"), (kv, "KV")):
            b.check_sentinels(f"{what} forward, {n}")
        out.o, out.lse = o.dense().double(), lse.dense().double()
    if backward:
        if not own:
            o, lse = Buf(io, dt, L.ldo, case.ref[0]), Buf(ilse, F32, 1, case.ref[1])
        do = Buf(io, dt, 0, case.do)
        dq, dkv = Buf(iq, dt, L.ldq), Buf(idkv, F32, L.lddkv, live=dkv_fill)
        bwd_args = (q.t[L.q_col0:], kv.t, o.t, do.t, lse.t, dq.t[L.q_col0:], dkv.t, B, H, N, M, L.ldq, L.ldkv, L.ldo, L.lddkv, L.k_off, L.v_off, case.scale)
        (ops.sr_attention_bwd_streamed if streamed else ops.sr_attention_bwd)(*bwd_args)
        ran(expected_bwd(M, dt, streamed))
        ran(planned(ops.attention_plan(*bwd_args, streamed=streamed)))
        torch.cuda.synchronize()
        for b, n in ((dq, "dQ"), (dkv, "dKV"), (o, "O"), (lse, "lse"), (do, "dO"), (q, "Q"), (kv, "KV")):
            b.check_sentinels(f"{what} backward, {n}")
        out.dq = dq.dense().double()
        out.dk, out.dv = dkv.dense().double().split(C, -1)
    return out


# ------------------------------------------------------------------------------------------------ the bars
def nearest_key(case, o_row, b, h):
    v = case.kv[b, :, case.C + h * HD: case.C + (h + 1) * HD].double()
    return int((v - o_row[None, :]).abs().amax(-1).argmin())


def where(case, b, h, n):
    kinds = ("selector", "repelled", "tail selector", "generic")
    return f"batch {b} head {h} query {n} ({kinds[int(case.kind[n])]}, selects key {int(case.pi[b, h, n])})"


def check_forward(case, out, parity, what, ref=None):
    ref_o, ref_lse = (ref or case.ref)[:2]
    dt, H = case.dtype, case.H
    vmax = float(case.kv[..., case.C:].abs().max())
    assert torch.isfinite(out.o).all() and torch.isfinite(out.lse).all(), f"{what}: non-finite O or lse"
    err = ac.heads((out.o - ref_o).abs(), H)                                   # [B,H,N,64]
    worst = int(err.amax(-1).argmax())
    b, h, n = worst // (H * case.N), worst // case.N % H, worst % case.N
    row = ac.heads(out.o, H)[b, h, n]
    assert parity(f"O/{what}", err.max(), TOL[dt] * vmax), (
        f"{what}: O off by {float(err.max()):.3e} (bar {TOL[dt] * vmax:.1e}) at {where(case, b, h, n)}; the output is nearest to V of key "
        f"{nearest_key(case, row, b, h)}; got {row[:6].tolist()} want {ac.heads(ref_o, H)[b, h, n, :6].tolist()}; last kernel {last_kernel()}")
    rel = (out.lse - ref_lse).abs() / ref_lse.abs().clamp_min(1.0)             # [B,H,N]
    worst = int(rel.argmax())
    b, h, n = worst // (H * case.N), worst // case.N % H, worst % case.N
    assert parity(f"lse/{what}", rel.max(), LSE_TOL[dt]), (
        f"{what}: lse {float(out.lse[b, h, n]):.6f}, want {float(ref_lse[b, h, n]):.6f} (bar {LSE_TOL[dt]:.0e} x max(1, |want|)) at {where(case, b, h, n)}")
    if dt == BF:
        # include/mvlt_hip.h: attn_fwd2_kernel sums its exponentials rounded to bf16 (8 significant bits: each within 2^-8 relative), so the sum is within
        # 2^-8 relative and lse within 2^-8 absolute of the exact one; 2^-20 |lse| for lse's own fp32 arithmetic.  The other forwards sum in fp32 and sit far inside.
        tight = (out.lse - ref_lse).abs() / (2.0 ** -8 + 2.0 ** -20 * ref_lse.abs())
        worst = int(tight.argmax())
        b, h, n = worst // (H * case.N), worst // case.N % H, worst % case.N
        assert parity(f"lse-abs/{what}", tight.max(), 1.0), (
            f"{what}: lse {float(out.lse[b, h, n]):.6f}, want {float(ref_lse[b, h, n]):.6f}: more than 2^-8 + 2^-20 |want| apart at {where(case, b, h, n)}")


def slice_error(got, ref, H):
    """max |err| of every (batch, head) slice over the slice's max |ref|: [B,H]; and the worst row of every slice"""
    e, r = ac.heads((got - ref).abs(), H), ac.heads(ref.abs(), H)
    return e.amax((-1, -2)) / r.amax((-1, -2)).clamp_min(1e-30), e.amax(-1).argmax(-1)


def check_backward(case, out, parity, what, ref=None):
    _, _, ref_dq, ref_dkv = ref or case.ref
    ref_dk, ref_dv = ref_dkv.split(case.C, -1)
    dt, H = case.dtype, case.H
    for name, got, want, row in (("dQ", out.dq, ref_dq, "query"), ("dK", out.dk, ref_dk, "key"), ("dV", out.dv, ref_dv, "key")):
        assert torch.isfinite(got).all(), f"{what}: non-finite {name}"
        rel, rows = slice_error(got, want, H)
        worst = int(rel.argmax())
        b, h = worst // H, worst % H
        assert parity(f"{name}/{what}", rel.max(), GRAD_TOL[dt]), (
            f"{what}: {name} off by {float(rel.max()):.3e} of the slice's maximum (bar {GRAD_TOL[dt]:.0e}) at batch {b} head {h} {row} {int(rows[b, h])}"
            + (f" ({where(case, b, h, int(rows[b, h]))})" if name == "dQ" else "") + f"; last kernel {last_kernel()}")


def check(case, out, parity, what, ref=None):
    check_forward(case, out, parity, what, ref)
    check_backward(case, out, parity, what, ref)


# ------------------------------------------------------------------------------------------------ A + B: decisive keys, every instantiation
@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", ac.LADDER_M)
def test_every_instantiation(ops, parity, dtype, M):
    """(1, 3, 77): three (batch, head) groups in a grid of eight (five idle workgroups per chunk), two whole query tiles and 13 queries; the
    public entry points (asserting the instantiation of the docstring's table) and the streamed exports on the same decisive case.  The
    backward reads the reference's O and lse here; test_backward_of_the_forwards_own_output composes it with the forward."""
    case = ac.decisive_case(1, 3, 77, M, dtype)
    for streamed in (False, True):
        check(case, run(ops, case, streamed), parity, "streamed" if streamed else "public")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", ac.LADDER_M)
def test_backward_of_the_forwards_own_output(ops, parity, dtype, M):
    """the composition the schedule runs: the backward reads the O and lse its forward wrote, same case and bars as test_every_instantiation.
    (bf16 M = 65..192 missed the dK bar with 3e-2..1e-1 while attn_fwd2_kernel summed unrounded numerators under bf16-rounded ones: a row decided by
    one key of its second block got O = V x bf16(e) / e, one bf16 ulp off an integer V, and D = rowsum(dO x O) carried that into dS and dK.)"""
    case = ac.decisive_case(1, 3, 77, M, dtype)
    for streamed in (False, True):
        check(case, run(ops, case, streamed, own=True), parity, "streamed" if streamed else "public")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", ac.LADDER_M)
def test_backward_across_query_chunks(ops, parity, dtype, M):
    """(1, 2, 200), backward only: more than one query chunk per (batch, head), so dK / dV meet in fp32 atomics"""
    case = ac.decisive_case(1, 2, 200, M, dtype)
    assert ops.sr_attention_bwd_chunks(1, 2, 200, M, dtype) > 1
    for streamed in (False, True):
        out = run(ops, case, streamed, forward=False)
        check_backward(case, out, parity, "streamed" if streamed else "public")


# ------------------------------------------------------------------------------------------------ C: layouts and guards
@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", [150, 385])
def test_strided_layout(ops, parity, dtype, M):
    """ldq = C + 64 behind a base pointer 64 columns in, ldkv = 2C + 32 with k_off 8 and v_off C + 16, ldo = C + 8, lddkv = 2C + 8: the live values
    meet the bars and every gap column and guard keeps its bits (run() checks them)"""
    case = ac.decisive_case(2, 2, 77, M, dtype)
    for streamed in (False, True):
        check(case, run(ops, case, streamed, layout=strided(case.C)), parity, "streamed" if streamed else "public")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("B,H,N,M", [(1, 3, 77, 150), (1, 3, 77, 385), (3, 1, 333, 150), (3, 1, 333, 385)])
def test_contiguous_layout_guards(ops, parity, dtype, B, H, N, M):
    """the schedule's layout with a guard row behind O, dQ and dKV and a guard element behind lse: idle workgroups (3 groups of 8) and the
    partial query tile (77 = 2 x 32 + 13, 333 = 10 x 32 + 13) leave them alone.  (run() guards every launch of this file, so the (1, 3, 77) cases
    repeat test_every_instantiation's layout at M = 150 / 385; they stay as the named guard cases, (3, 1, 333) adds eleven query tiles and B > 1.)"""
    case = ac.decisive_case(B, H, N, M, dtype)
    for streamed in (False, True):
        check(case, run(ops, case, streamed), parity, "streamed" if streamed else "public")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("B,H,N,M", [(2, 3, 50, 29), (1, 5, 64, 150), (2, 3, 50, 225), (1, 3, 33, 272), (2, 3, 100, 385)])
def test_one_chunk_fp32_dkv_needs_no_zero_fill(ops, parity, dtype, B, H, N, M):
    """include/mvlt_hip.h: with one query chunk per (batch, head) every dKV element is stored exactly once -- an fp32 dKV full of NaN comes back
    finite and within the bars (resident kernels, the streamed kernel past the resident range, and the streamed export where it has one chunk)"""
    case = ac.decisive_case(B, H, N, M, dtype)
    assert ops.sr_attention_bwd_chunks(B, H, N, M, dtype) == 1
    check(case, run(ops, case, dkv_fill=math.nan), parity, "public")
    if N <= 128:                                                   # the streamed backward: one chunk up to 128 queries
        check(case, run(ops, case, streamed=True, dkv_fill=math.nan), parity, "streamed")


# ------------------------------------------------------------------------------------------------ D: numeric edges
# (dtype, M, streamed): five forward + backward pairs reach the six families, each tuple a forward AND a backward family -- round-3 forward + DMA backward; resident bf16 forward
# (+ DMA backward again); resident fp32 forward + resident fp32 backward; streamed forward + streamed backward, in bf16 and in fp32
FAMILIES = [(BF, 100, False), (BF, 272, False), (F32, 100, False), (BF, 100, True), (F32, 100, True)]


@pytest.mark.parametrize("scale", [1.0, 0.03125, 0.1])
@pytest.mark.parametrize("dtype,M,streamed", FAMILIES, ids=[f"{DT_ID[d]}-M{M}-{'streamed' if s else 'public'}" for d, M, s in FAMILIES])
def test_scale(ops, parity, scale, dtype, M, streamed):
    """every test before this one passed scale = 0.125: N(0,1) V and dO, Q and K scaled so that the scaled scores stay N(0,1)"""
    case = ac.with_reference(ac.generic(2, 3, 77, M, dtype, seed=3, scale=scale))
    check(case, run(ops, case, streamed), parity, f"scale {scale}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("streamed", [False, True], ids=["public", "streamed"])
def test_single_key(ops, parity, dtype, streamed):
    """M = 1 on integer data: the softmax is 1, so O = V[0], lse = the score, dQ = 0, dK = 0 and dV[0] = sum of dO (exactly, in fp32)"""
    B, H, N = 2, 3, 77
    g = torch.Generator(device="cpu").manual_seed(5)
    ints = lambda *s: torch.randint(-3, 4, s, generator=g).to(dtype)
    case = types.SimpleNamespace(B=B, H=H, N=N, M=1, C=H * HD, dtype=dtype, scale=ac.SCALE, kind=torch.full((N,), 3), pi=torch.full((B, H, N), -1),
                                 q=ints(B, N, H * HD), kv=ints(B, 1, 2 * H * HD), do=ints(B, N, H * HD))
    k, v = case.kv.double().split(case.C, -1)
    score = ac.heads(case.q.double() * k, H).sum(-1) * case.scale                                        # [B,H,N]
    dv = case.do.double().sum(1, keepdim=True)
    closed = (v.expand(B, N, case.C), score, torch.zeros(B, N, case.C, dtype=torch.float64), torch.cat((torch.zeros_like(dv), dv), -1))
    case.ref = closed
    out = run(ops, case, streamed)
    check_forward(case, out, parity, "M=1")
    # dQ and dK are zero: the bars' normaliser is the magnitude of the operands (integers up to 3), dV's its own maximum
    assert torch.isfinite(out.dq).all() and torch.isfinite(out.dk).all() and torch.isfinite(out.dv).all()
    assert parity("dQ/M=1", out.dq.abs().max(), GRAD_TOL[dtype] * 3) and parity("dK/M=1", out.dk.abs().max(), GRAD_TOL[dtype] * 3)
    rel, rows = slice_error(out.dv, dv, H)
    assert parity("dV/M=1", rel.max(), GRAD_TOL[dtype])
    if dtype == F32:
        assert torch.equal(out.dv, dv), f"fp32 dV[0] != sum of dO: max difference {float((out.dv - dv).abs().max()):.3e}"


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", [33, 150, 385])
def test_single_query(ops, parity, dtype, M):
    """N = 1: one live row in the only query tile.  N(0,1) data: the one query of the decisive inputs is a selector, whose saturated softmax has dQ = dK = 0
    and so no scale to judge them against (M = 1 is test_single_key)"""
    case = ac.with_reference(ac.generic(2, 3, 1, M, dtype, seed=4, scale=ac.SCALE))
    for streamed in (False, True):
        check(case, run(ops, case, streamed), parity, "streamed" if streamed else "public")


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", [29, 192, 320, 385])
def test_zero_queries_give_the_mean(ops, parity, dtype, M):
    """all-equal scores: O = mean(V) and lse = log M in closed form; the backward against the float64 autograd"""
    base = ac.decisive(2, 3, 77, M, dtype, seed=1)
    case = ac.with_reference(types.SimpleNamespace(**{**vars(base), "q": torch.zeros_like(base.q), "kind": torch.full((77,), 3), "pi": torch.full((2, 3, 77), -1)}))
    mean = case.kv[..., case.C:].double().mean(1, keepdim=True).expand(2, 77, case.C)
    closed = (mean, torch.full((2, 3, 77), math.log(M), dtype=torch.float64)) + tuple(case.ref[2:])
    for streamed in (False, True):
        check(case, run(ops, case, streamed), parity, "streamed" if streamed else "public", ref=closed)


@pytest.mark.parametrize("dtype", [BF, F32], ids=DT_ID.get)
@pytest.mark.parametrize("M", [150, 272, 385])
def test_large_scores(ops, parity, dtype, M):
    """selector amplitude 1024: scaled scores of +-1408 in steps of 256, exp-space differences far past fp32's range -- the bare v_exp_f32 and
    every rescale branch.  The first query tile selects keys of the first 32, the second keys of the last tile, the third alternates: the round-3
    forward's `second block tops the first by 2^24` branch (wave-uniform) is taken by one wave, not by another, and by half the lanes of a third.
    Bars: the fp32 products s x scale x log2(e) near 2031 and lse near 1408 carry roundings of ~6e-5 each, so P = exp(s scale - lse) is good to
    ~2e-4 in any fp32 evaluation -- inside GRAD_TOL of either dtype, so the gradients are held to the usual bars too."""
    N = 77
    i = torch.arange(N)
    first, last = (i * 7) % min(32, M), ac.last_tile(M) + (i * 5) % (M - ac.last_tile(M))
    pi = torch.where(i < 32, first, torch.where(i < 64, last, torch.where(i % 8 < 4, first, last)))
    case = ac.with_reference(ac.decisive(2, 3, N, M, dtype, seed=2, amp=1024.0, pi=pi))
    assert float(case.ref[1].abs().max()) > 1400.0
    for streamed in (False, True):
        check(case, run(ops, case, streamed), parity, "streamed" if streamed else "public")
