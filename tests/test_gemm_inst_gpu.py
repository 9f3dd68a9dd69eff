"""GPU: every compiled GEMM instantiation that no bench shape and no other test reaches, run on exact integer data against a float64 reference, bit for bit (the
GELU epilogues: exact where the unit is on, within the derived off-side bound of tests/mlp_cases.py where it is off), kernel name asserted after every launch,
guard rows and columns asserted untouched.  The cases: tests/gemm_inst_cases.py; their plans and premises: tests/test_gemm_inst_cpu.py; the table:
docs/gemm_instantiations.md."""
import pytest

from tests import gemm_inst_cases as gi
from tests.gemm_inst_cases import last_kernel, ran
from tests.test_exact_gpu import ops          # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

SEEN = {}                                     # case id -> the kernel the library launched for it


def run(ops, case):
    t = case.make()
    assert gi.plan(t).name == case.kernel
    gi.launch(ops, t)
    ran(gi.BIG_FAMILY if case.kernel == gi.BIG_KERNEL else case.kernel)
    SEEN[case.id] = last_kernel()
    assert SEEN[case.id] == case.kernel, f"meant to reach {case.kernel}, the library launched {SEEN[case.id]}"
    gi.check(t)


def cases(group):
    return pytest.mark.parametrize("case", gi.group(group), ids=[c.id for c in gi.group(group)])


@cases("epi0")
def test_generic_epilogue_behind_a_gather(ops, case):
    """row_scale without R (factors {0, 0.5, 1, 2}, one per image, several inside one 128-row tile), bias, ragged M and N, behind the patch and the 3x3 gather"""
    run(ops, case)


@cases("epi2")
def test_residual_behind_a_patch_gather(ops, case):
    """R in an fp32 buffer of its own beside an fp32 C; R aliasing a bf16 C under a row factor"""
    run(ops, case)


@cases("epi5")
def test_column_statistics_behind_a_patch_gather(ops, case):
    """fp32 and fp16 C, four interleaved accumulators: C, the column sums and the sums of squares all exact"""
    run(ops, case)


@cases("scatter")
def test_scatter_behind_a_gather(ops, case):
    """EPI 6 / 7: the input-gradient scatter through a patch map that is not the gather's; the text rows keep their fill, EPI 7 adds to what the buffer held"""
    run(ops, case)


@cases("act")
def test_gelu_epilogues_behind_a_gather(ops, case):
    """EPI 3 / 4 on saturated pre-activations of the gathered operand (and on plain rows at N <= 64): H exact, G and dH exact on the on side and within bound_G /
    bound_dH on the off side"""
    run(ops, case)


@cases("halo")
def test_conv3x3_halo_tiles(ops, case):
    """conv3_nt_kernel<16, 192, 1>, <64, 128, 1> and <64, 128, 5> on three images of three tiles each: interior tiles, idle workgroups, a ragged column tile"""
    run(ops, case)


@cases("tn")
def test_tn_lds_dma_tiles_behind_mapped_rows(ops, case):
    """the 128 x 64 and the 64 x 128 tile with batch-strided rows and behind a patch gather: accumulate into a filled C, colsum_a, two m-splits, ragged last k-tile"""
    run(ops, case)


@cases("big")
def test_tn_bf16_register_staged_128_wide(ops, case):
    """gemm_tn_kernel<bf16, 128> at M = 2^24 rows, N1 = 8, N2 = 72: A is 268 MB and B 2.4 GB on the device (a 4096-row block repeated)"""
    run(ops, case)


def test_the_kernels_seen_are_the_claimed_set():
    """when every case above ran in this process: the names the library reported are exactly the claimed ones"""
    if len(SEEN) == len(gi.CASES):
        assert set(SEEN.values()) == gi.CLAIMED
