"""GPU: GELU and GELU' element by element through the four 8-phase NT GEMM instantiations that carry them -- gemm_nt_p8_kernel<3 | 4, 4 | 3, 2, 2, false>, the
fc1 + GELU and the x gelu'(H) launches of the stage 3-4 MLPs (tests/gelu_cases.py builds the operands, tests/test_gelu_cases_cpu.py pins their premises and
shows that each move of a wrong epilogue is caught; docs/gelu_range.md has the argument and the measured margins).  They compile nt_epilogue_lean with four wave
columns, four or THREE 32-row halves behind a two-slot prefetch of H, no bound checks and staging in the LDS the K-loop has just left: every output element is one
activation of a known input, compared on the device with the float64 exact-erf GELU (or its autograd derivative) under the polynomial form's bar.  The shapes are the
smallest the plan sends there (200 tiles of 256 x 256, 192 tiles of 192 x 256); the references are 67 x 128 tables indexed on the device."""
import pytest
import torch

from tests import gelu_cases as gc
from tests.test_exact_gpu import dev, last_kernel, ops                 # noqa: F401  (ops is the module-scoped fixture)
from tests.test_gelu_range_gpu import SENTINEL, guarded, put, untouched

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TILES = sorted(gc.P8_M)
FORM = "poly"                                                         # gelu_fast2 / gelu_fast_grad2 as this tree compiles them (pinned by tests/test_gelu_cases_cpu.py)


def launch(ops, A, B, out, c, act, *, H, bias=None, ld=None, ldc=None, c_map=None):
    """one launch; the plan names the instantiation of this tile and act, and that is what ran"""
    ld, ldc = ld or c.K, ldc or c.N
    args = (A, B, out, c.M, c.N, c.K, ld, ld, ldc)
    kw = dict(act=act, H=H, bias=bias, c_map=c_map)
    ops.gemm_nt(*args, **kw)
    assert ops.gemm_nt_plan(*args, **kw).name == last_kernel() == gc.P8_KERNEL[c.BM] % (2 + act), last_kernel()


def sweep_h(c, u):
    """the table's values at u as the host writes them: bf16 on the device"""
    return c.t2.h.to(dev())[u].to(BF)


def outputs(c):
    cbuf, C = guarded((c.M, c.N), BF, SENTINEL)
    hbuf, H = guarded((c.M, c.N), BF, SENTINEL)
    return cbuf, C, hbuf, H


@pytest.mark.parametrize("BM", TILES)
def test_p8_sweep_gelu(ops, parity, BM):
    """case 1, EPI 3: A[m][0] = a_(m mod 67), B[n][0] = w_(n mod 128), K = 128, no bias: the stored H is the tiled sweep bit for bit, C = bf16(gelu~(h)) within the bar
    of every element (67 is coprime to every tile dimension: every wave, lane, register and half sees many inputs)"""
    c = gc.p8_sweep_case(BM)
    cbuf, C, hbuf, H = outputs(c)
    launch(ops, put(c.A), put(c.B), C, c, 1, H=H)
    gc.p8_check_h(c, H, f"H {BM}")
    parity(f"{FORM} g/p8 {BM} sweep", gc.p8_check_act1(c, C, f"sweep act 1, tile {BM}"), 1.0)
    untouched(cbuf, "C"), untouched(hbuf, "H")


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("BM", TILES)
def test_p8_sweep_gelu_grad(ops, parity, BM, with_bias):
    """case 2, EPI 4: H = the tiled sweep from the host, A[m][1] = 2^(m mod 3), B[n][1] = 2^-(n mod 5): C = bf16(acc gelu'~(h)) with an accumulator that names its row and
    its column, so an accumulator paired with the H of another half, row or chunk is over the bar.  With a bias: mvlt_gemm_nt adds the bias to the product BEFORE the
    activation step of either act, so act 2 means C = (A B^T + bias) gelu'(H) (the generic epilogue and the lean ones agree).  The trunk never passes one: its act 2
    launches are the fc1 input gradients dG W2 x gelu'(H), which have no bias term; the case pins what the ABI does with one."""
    c = gc.p8_sweep_case(BM)
    bias = c.bias2 if with_bias else None
    Hin = sweep_h(c, c.u2(dev()))
    keep = Hin.clone()
    cbuf, C = guarded((c.M, c.N), BF, SENTINEL)
    launch(ops, put(c.A2), put(c.B2), C, c, 2, H=Hin, bias=None if bias is None else put(bias, torch.float32))
    parity(f"{FORM} dg/p8 {BM} sweep{' + bias' if with_bias else ''}", gc.p8_check_act2(c, C, f"sweep act 2, tile {BM}, bias {with_bias}", bias), 1.0)
    untouched(cbuf, "C")
    assert torch.equal(Hin.view(torch.int16), keep.view(torch.int16)), "act 2 wrote H"


@pytest.mark.parametrize("BM", TILES)
def test_p8_bias_only_gelu(ops, parity, BM):
    """case 3, EPI 3: A = 0 and bias[n] = a sweep value by (37 n + 11) mod 2048 -- no period of 64 or 128 columns, so the per-lane bias chunk of each of the four wave
    columns is pinned, which the rank-one sweep (period 128) cannot do.  H[m][n] = bf16(bias[n]) bit for bit and C within the bar in EVERY row; four launches carry all
    8192 values"""
    A = B = None
    for rep in range(4):
        c = gc.p8_bias_case(BM, rep)
        if A is None:
            A, B = put(c.A), put(c.B)
        cbuf, C, hbuf, H = outputs(c)
        launch(ops, A, B, C, c, 1, H=H, bias=put(c.bias, torch.float32))
        gc.p8_check_h(c, H, f"H {BM} bias {rep}")
        parity(f"{FORM} g/p8 {BM} bias {rep}", gc.p8_check_act1(c, C, f"bias only, tile {BM}, launch {rep}"), 1.0)
        untouched(cbuf, "C"), untouched(hbuf, "H")


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("BM", TILES)
def test_p8_position(ops, parity, BM, act):
    """case 4, K = 192 (three k-tiles: the odd count), A and B in {-1, 0, 1}: the whole K-loop feeds the epilogue.  act 1: h = A B^T is an integer, H == h bit for bit and
    C within the bar of GELU(h) (the form's worst E).  act 2: H = a sweep value per (m, n) with no period, acc = the integer product, C against acc gelu'(H).  A refill,
    a fragment or an H row in the wrong place fails here at the element's bar, not at 2e-2.  Each launch runs twice: bit-identical"""
    c = gc.p8_position_case(BM)
    A, B = put(c.A), put(c.B)
    Hin = sweep_h(c, c.u2(dev())) if act == 2 else None
    keep = Hin.clone() if act == 2 else None
    runs = []
    for _ in range(2):
        cbuf, C = guarded((c.M, c.N), BF, SENTINEL)
        hbuf, H = guarded((c.M, c.N), BF, SENTINEL) if act == 1 else (None, Hin)
        launch(ops, A, B, C, c, act, H=H)
        untouched(cbuf, "C")
        if act == 1:
            untouched(hbuf, "H")
        runs.append((C, H.clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16)), "launch-to-launch difference"
    C, H = runs[0]
    if act == 1:
        gc.p8_check_h(c, H, f"H {BM} position")
        parity(f"{FORM} g/p8 {BM} position", gc.p8_check_act1(c, C, f"position act 1, tile {BM}"), 1.0)
    else:
        assert torch.equal(H.view(torch.int16), keep.view(torch.int16)), "act 2 wrote H"
        parity(f"{FORM} dg/p8 {BM} position", gc.p8_check_act2(c, C, f"position act 2, tile {BM}"), 1.0)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("BM", TILES)
def test_p8_layout(ops, parity, BM, act):
    """case 4 once more per act with lda = ldb = K + 8 (the pad poisoned), ldc = 2056 with H at the same stride, and a batch-strided c_map.  The epilogue addresses H
    through the SAME map and stride as C (one index for both), so H is read (act 2) and stored (act 1) at the mapped rows; sentinel columns, the rows between the
    batches and the guard rows come back unchanged"""
    from mvlt_amd._lib import rowmap
    c = gc.p8_position_case(BM)
    nb, rows = gc.P8_BATCH[BM]
    stride, off, ldc, ld = rows + 40, 24, c.N + 8, c.K + 8
    assert nb * rows == c.M

    def padded(t):
        out = torch.full((t.shape[0], ld), SENTINEL, device=dev(), dtype=BF)
        out[:, :c.K] = put(t)
        return out
    phys = (torch.arange(nb, device=dev())[:, None] * stride + off + torch.arange(rows, device=dev())[None, :]).reshape(-1)
    written = torch.zeros(nb * stride, ldc, dtype=torch.bool, device=dev())
    written[phys, :c.N] = True
    cbuf, C = guarded((nb * stride, ldc), BF, SENTINEL)
    hbuf, H = guarded((nb * stride, ldc), BF, SENTINEL)
    if act == 2:
        H[phys, :c.N] = sweep_h(c, c.u2(dev()))
        keep = hbuf.clone()
    launch(ops, padded(c.A), padded(c.B), C, c, act, H=H, ld=ld, ldc=ldc, c_map=rowmap(rows, stride, off))
    got = C[phys, :c.N]
    if act == 1:
        gc.p8_check_h(c, H[phys, :c.N], f"H {BM} layout")
        parity(f"{FORM} g/p8 {BM} layout", gc.p8_check_act1(c, got, f"layout act 1, tile {BM}"), 1.0)
        assert bool((H[~written] == SENTINEL).all()), "H: written outside the mapped rows and the N columns"
    else:
        parity(f"{FORM} dg/p8 {BM} layout", gc.p8_check_act2(c, got, f"layout act 2, tile {BM}"), 1.0)
        assert torch.equal(hbuf.view(torch.int16), keep.view(torch.int16)), "act 2 wrote H"
    assert bool((C[~written] == SENTINEL).all()), "C: written outside the mapped rows and the N columns"
    untouched(cbuf, "C"), untouched(hbuf, "H")
