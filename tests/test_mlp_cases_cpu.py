"""CPU: the premises of the exact fused-MLP cases (tests/mlp_cases.py), which tests/test_mlp_exact_gpu.py relies on without re-checking: every reference is
an integer grid below 2^24, every value a kernel keeps in bf16 is bf16-exact, what the off units may add stays below a quarter, and each case reaches
the loop it is named after.  The last tests perturb the REFERENCE the way a wrong kernel would and show that the comparison names the element."""
import re

import pytest
import torch

from tests import mlp_cases as mc

FWD = [pytest.param(*a, id=f"C{a[0]}-hid{a[1]}-{'h' if a[2] else 'n'}-M{a[4]}-{'off' if a[7] else 'on'}") for a in mc.FWD_CASES]
WG = [pytest.param(*a, id=f"{a[0]}-{'scaled' if a[4] else 'plain'}") for a in mc.WG_CASES]
R2 = [pytest.param(*a, id=f"C{a[0]}-hid{a[1]}-rps{a[2]}") for a in mc.R2_CASES]
OUTS = ("out", "h", "dx", "dw1", "db1", "dw2", "db2")


def grid(t, unit=1.0):
    q = t / unit
    return torch.equal(q, q.round()) and float(q.abs().max()) < mc.LIM


def common(c, bounded):
    """`bounded`: the outputs the case's kernels compute, whose off-unit bounds must hold (the forward and dx cases launch no weight-gradient kernel)"""
    r = c.ref
    unit = 0.5 if c.scale is not None and bool((c.scale == 0.5).any()) else 1.0      # a factor of 0.5 makes halves, nothing else does
    for k in OUTS:
        assert grid(getattr(r, k), unit), f"{k} is no grid of {unit} below 2^24"
    assert set(c.srow.unique().tolist()) <= {0.0, 0.5, 1.0, 2.0}
    # point 3: what the kernels hold as bf16 on the way -- the pre-activation, dG, and both times the DropPath factor (the per-row weight-gradient kernel)
    assert grid(r.h) and mc.SAT <= float(r.h.abs().min()) and float(r.h.abs().max()) <= 256
    assert grid(r.dG) and float(r.dG.abs().max()) <= 256
    for t in (r.h * c.srow, r.dG * c.srow):
        assert mc.bf16_exact(t) and float(t.abs().max()) <= 256
    assert bool((r.on == (c.b1 > 0).double()).all()), "a unit is on for one row and off for another"
    assert c.off == bool((c.b1 < 0).any())
    for k in bounded:
        b = getattr(c.bound, k)
        assert float(b.max()) <= 0.25, (k, float(b.max()))
        assert c.off or float(b.max()) == 0.0
    if c.off:
        off = mc.off_units(c.hid)
        for s in range(c.hid // 32):                       # every 32-unit slice holds both kinds, and so does every position of a lane's 8 consecutive units
            assert 0 < int(off[32 * s: 32 * s + 32].sum()) < 32
        for p in range(8):
            assert 0 < int(off[p::8].sum()) < c.hid // 8


@pytest.mark.parametrize("C,hid,h_out,fam,M,rps,factors,off", FWD)
def test_forward_and_dx_case(C, hid, h_out, fam, M, rps, factors, off):
    c = mc.fwd_case(C, hid, M, rps, factors, off)
    common(c, ("out", "dx"))
    assert mc.bf16_exact(c.ref.dx) and float(c.ref.dx.abs().max()) <= 256, "dx is rounded by its bf16 store"
    assert (fam == "mlp_pipe_kernel") == (not h_out and hid >= 128)        # the rule of choose() in csrc/mlp_plan.h, restated
    fwd, dx = mc.planned("fwd", C, hid, M, h_out=h_out, rps=rps), mc.planned("bwd_dx", C, hid, M, rps=rps)
    assert fwd is None or (fwd.name, dx.name) == (f"{fam}<{C}, 0>", f"{'mlp_fused_kernel' if hid < 128 else 'mlp_pipe_kernel'}<{C}, 1>")


def check_partials(c):
    for z, p1, p2 in mc.split_partials(c):
        for p in (p1, p2):
            assert mc.bf16_exact(p) and float(p.abs().max()) <= 256, f"a partial tile of split {z} is not bf16-exact"
            assert grid(p) or (grid(p, 0.5) and float(p.abs().max()) <= 128)


@pytest.mark.parametrize("name,C,hid,M,scaled", WG)
def test_weight_gradient_case(name, C, hid, M, scaled):
    c = mc.wg_case(C, hid, M, scaled)
    common(c, ("dw1", "db1", "dw2"))
    check_partials(c)
    sp = mc.wgrad_split(C, hid, M)
    assert (c.rps % 64 == 0), "the tile-uniform kernel"
    p = mc.planned("bwd_dw", C, hid, M, rps=c.rps)
    assert p is None or (p.name, p.m_per_split, p.splits) == (f"mlp_wgrad2_kernel<{C}, {4 if C == 64 else 8}>", sp.m_per_split, sp.splits)
    if name.startswith("single"):
        assert sp.tiles == 1
        return
    assert name.startswith("multi-tile") and sp.tiles >= 2 and sp.splits % 8 != 0 and sp.idle > 0
    if sp.tiles == 2:
        assert M - (sp.splits - 1) * sp.m_per_split == 17, "a 17-row last split: its second tile is all zero page"
    if not scaled:
        return
    per_split = [c.scale[z * sp.tiles: (z + 1) * sp.tiles].tolist() for z in range(sp.splits)]
    assert any(len({f for f in fs if f != 0}) >= 2 for fs in per_split), "two different non-zero factors inside one split: the rescale branch"
    assert all(f == 0 for f in per_split[mc.DROPPED_SPLIT]) and len(per_split[mc.DROPPED_SPLIT]) == sp.tiles, "one split entirely dropped"
    assert any(fs[0] == 0 and fs[1] != 0 for fs in per_split if len(fs) > 1), "a dropped tile in front of the first live one"
    if sp.tiles >= 3:
        assert any(fs[0] != 0 and fs[1] == 0 and fs[2] != 0 and fs[0] != fs[2] for fs in per_split if len(fs) == 3), "a dropped tile between two live ones"


def test_multi_tile_cases_reach_two_and_three_tiles():
    tiles = {name: mc.wgrad_split(C, hid, M) for name, C, hid, M in mc.WG_MULTI}
    assert all(t.tiles >= 2 for t in tiles.values()) and max(t.tiles for t in tiles.values()) >= 3
    assert (tiles["multi-tile-64-4241"].splits, tiles["multi-tile-128-2193"].splits) == (34, 18)
    assert mc.wgrad_split(64, 512, 1344).tiles == 1, "the largest case of test_fused_mlp stays at one tile per split"


@pytest.mark.parametrize("C,hid,rps,factors", R2)
def test_per_row_factor_case(C, hid, rps, factors):
    c = mc.r2_case(C, hid, rps, factors)
    common(c, ("dw1", "db1", "dw2"))
    assert rps % 64 != 0 and c.scale is not None, "the per-row kernel"
    p = mc.planned("bwd_dw", C, hid, c.M, rps=rps)
    assert p is None or p.name == f"mlp_wgrad_kernel<{C}>"
    samples = [len(set(range(t, min(t + 64, c.M))[i] // rps for i in range(min(64, c.M - t)))) for t in range(0, c.M, 64)]
    if rps == 100:
        assert max(samples) == 2
    if rps == 52:
        rows = range(256, 320)
        assert sorted({m // rps for m in rows}) == [4, 5, 6] and len({factors[4], factors[5], factors[6]}) == 3
    if rps == 20:
        assert max(samples) >= 4


# ---------------------------------------------------------------------------------------------------------------- the comparison notices
def located(fn, row=None, col=None):
    with pytest.raises(AssertionError) as e:
        fn()
    msg = str(e.value)
    assert "(row, col, got, want)" in msg
    first = re.search(r"\[\((\d+), (\d+), ", msg)
    assert first is not None
    if row is not None:
        assert int(first.group(1)) == row, msg
    if col is not None:
        assert int(first.group(2)) == col, msg
    return msg


@pytest.mark.parametrize("off", [False, True])
def test_comparison_fails_on_a_dropped_row_a_swapped_pair_and_a_wrong_factor(off):
    c = mc.fwd_case(64, 192, 200, 50, (2.0, 0.0, 0.5, 1.0), off)
    r, b = c.ref, c.bound
    mc.compare(r.out.float(), r.out, b.out, "out")                       # the reference itself passes, as fp32 and rounded to bf16
    mc.compare(r.out.float().to(mc.BF), r.out, b.out, "out_op")
    mc.compare(r.dx.float().to(mc.BF), r.dx, b.dx, "dx")
    # one dropped row: row 37 of x read as zeros
    x = c.x.double().clone()
    x[37] = 0
    p = mc.reference(c, x=x)
    located(lambda: mc.compare(p.out.float(), r.out, b.out, "out"), row=37)
    located(lambda: mc.compare(p.h.float().to(mc.BF), r.h, None, "h_out"), row=37)
    located(lambda: mc.compare(p.dw1.float(), r.dw1, b.dw1, "dw1"))
    # two hidden units exchanged between fc1 and fc2 (both on: the smallest possible misplacement)
    on = (c.b1 > 0).nonzero().flatten().tolist()
    p = mc.reference(c, swap=(on[3], on[4]))
    located(lambda: mc.compare(p.out.float(), r.out, b.out, "out"))
    located(lambda: mc.compare(p.dw2.float(), r.dw2, b.dw2, "dw2"), col=min(on[3], on[4]))
    # one row under its neighbour sample's factor: row 150 (sample 3, factor 1) takes sample 2's 0.5
    srow = c.srow.clone()
    srow[150] = 0.5
    p = mc.reference(c, srow=srow)
    located(lambda: mc.compare(p.out.float(), r.out, b.out, "out"), row=150)
    located(lambda: mc.compare(p.dx.float().to(mc.BF), r.dx, b.dx, "dx"), row=150)
    located(lambda: mc.compare(p.db2.float(), r.db2, None, "db2"))


def test_comparison_fails_on_the_third_sample_of_a_tile():
    """what mlp_wgrad_kernel computed before its factor lookup went per row: rows of the THIRD sample inside a 64-row tile under the second sample's factor"""
    C, hid, rps, factors = mc.R2_CASES[1]
    c = mc.r2_case(C, hid, rps, factors)
    srow = c.srow.clone()
    srow[312:320] = factors[5]                              # tile [256, 320): rows 312.. belong to sample 6
    p = mc.reference(c, srow=srow)
    for k in ("dw1", "db1", "dw2", "db2"):
        located(lambda: mc.compare(getattr(p, k).float(), getattr(c.ref, k), getattr(c.bound, k), k))


def test_an_activation_off_by_one_unit_moves_a_result_by_at_least_one():
    c = mc.fwd_case(128, 128, 129, 50, (0.5, 2.0, 1.0), True)
    flipped = mc.NS(**vars(c))
    flipped.b1 = -c.b1                                     # on and off exchanged
    p = mc.reference(flipped)
    d = (p.out - c.ref.out).abs()
    assert float(d[d > 0].min()) >= 0.5 and float(d.max()) >= 1.0
    located(lambda: mc.compare(p.out.float(), c.ref.out, c.bound.out, "out"))
