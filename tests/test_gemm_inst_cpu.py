"""CPU: the cases of tests/gemm_inst_cases.py without a device -- every case plans the instantiation it claims, the claimed names cover every instantiation that
tests/test_gemm_plan_cpu.py lists as unrecorded (but the one no argument struct reaches), the premises of the references hold, and the comparison notices a
reference computed the way a wrong kernel would compute it."""
import pytest
import torch

from tests import gemm_inst_cases as gi
from tests import mlp_cases as mc
from tests.test_gemm_plan_cpu import UNRECORDED, _switch_instantiations

CPU = torch.device("cpu")
IDS = [c.id for c in gi.CASES]


@pytest.fixture(scope="module")
def built():
    """every case built once on the CPU"""
    with gi.on_device(CPU):
        return {c.id: c.make() for c in gi.CASES}


def test_the_claimed_names_cover_the_unrecorded_instantiations():
    compiled = set(_switch_instantiations())
    assert gi.CLAIMED <= compiled and len(IDS) == len(set(IDS))
    assert gi.UNREACHABLE in UNRECORDED and gi.UNREACHABLE not in gi.CLAIMED
    assert gi.CLAIMED >= set(UNRECORDED) - {gi.UNREACHABLE}
    assert gi.CLAIMED == set(UNRECORDED) - {gi.UNREACHABLE}                     # ... and nothing else: every other instantiation has a recorded launch
    assert gi.ALREADY_RUN <= gi.CLAIMED and len(gi.CLAIMED - gi.ALREADY_RUN) == 30
    assert {c.group for c in gi.CASES} == set(gi.GROUPS)


@pytest.mark.parametrize("cid", IDS)
def test_every_case_plans_the_kernel_it_claims(built, cid):
    case, t = next(c for c in gi.CASES if c.id == cid), built[cid]
    p = gi.plan(t)
    assert p.name == case.kernel, (cid, p.name)
    assert p.fold == 0 and p.swap_operands == 0
    if case.group == "halo":                                                  # 9 row tiles in whole groups of 8: 16 workgroups per column tile, 7 idle
        assert p.grid == [16, 1, 1]
    if case.group == "tn":
        assert p.splits == 2 and p.per_split % 64 == 0 and t.args[3] % 64 != 0
    if case.group == "big":
        assert p.grid == [1, 1, 1024] and t.args[3] == 1 << 24


@pytest.mark.parametrize("cid", IDS)
def test_premises_of_every_case(built, cid):
    case, t = next(c for c in gi.CASES if c.id == cid), built[cid]
    for what, got, ref, bound, gelu in t.outs:
        if not gelu:
            gi.integral(ref, 0.5)
        else:
            assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 256 and mc.bf16_exact(ref), what     # integers a bf16 tile holds exactly
        assert got().shape == ref.shape
    for what, ok in t.guards:
        assert bool(ok().all()), what                                           # (the fills are in place before the launch)
    if case.group == "act":
        c = t.sat
        assert float(c.h.abs().min()) >= mc.SAT and bool((c.on == 1).any()) and bool((c.on == 0).any())
        assert c.h.shape == (t.args[3], t.args[4])                              # h is the product of the GATHERED operand: M rows of the map
        assert float(c.bound_G.max()) <= 256 * mc.EPS_PHI and float(c.bound_dH.max()) <= 256 * mc.EPS_DG
    if case.group == "halo":
        assert t.tiles_per_img >= 3 and t.args[3] % 128 == 0
    if case.group == "epi0":
        first_tile = t.srow[:128, 0]
        assert t.rps % 128 != 0 and 128 % t.rps != 0 and len(set(first_tile.tolist())) >= 2
    if case.group == "scatter":
        assert t.text_rows > 0 and t.kw["c_map"].w_out != getattr(t.kw.get("a_map"), "w_out", -1)
    for key, X in (("a_map", t.args[0]), ("b_map", t.args[1])):                 # text tokens holding 99 behind the image tokens of every gathered operand
        m = t.kw.get(key)
        if m is not None and m.mode != 0:
            assert _text(m) > 0 and int((X == gi.TEXT).all(1).sum()) == X.shape[0] // m.tokens_in * _text(m)


def _text(m):
    """text tokens behind the image tokens of one image of a gather map"""
    return m.tokens_in - (m.h_in * m.w_in if m.mode == 2 else m.r * m.r * m.hw_out)


@pytest.mark.parametrize("cid", IDS)
def test_the_comparison_notices_a_wrong_kernel(built, cid):
    """a right kernel's output (the reference rounded once to the output's type) passes; the same output against the reference of a kernel with one halo row from the
    zero page / the scatter map's w_out off by one / a neighbour's row factor / the residual added twice fails"""
    case, t = next(c for c in gi.CASES if c.id == cid), built[cid]
    with gi.on_device(CPU):
        wrong = case.make(perturb=case.perturb)
    noticed = 0
    for (what, got, ref, bound, gelu), (_, _, wref, wbound, _) in zip(t.outs, wrong.outs):
        out = gi.rounded(ref, got())
        if gelu:
            mc.compare(out, ref, bound, what)
        else:
            gi.exact(out, ref, what)
        try:
            if gelu:
                mc.compare(out, wref, wbound, what)
            else:
                gi.exact(out, wref, what)
        except AssertionError:
            noticed += 1
    assert noticed >= 1, (cid, case.perturb)
    assert {c.perturb for c in gi.CASES} == {"halo", "w_out", "factor", "r_twice"}
