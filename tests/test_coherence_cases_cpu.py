"""CPU: the premises of tests/coherence_cases.py.  `audit` passes a stand-in store whose copies come from the definitions, and names the copy and the
element of every staleness planted in it -- one element of C, of ::T, of the ::T padding, of ::K / ::KT / ::F, of the two score copies, of a folded
weight and of a folded shift.  The definitions themselves are held against torch: ::K against the weight layout F.unfold implies, ::F against the
weight of conv_transpose2d, the fold against F.batch_norm(F.conv2d(...)) in eval mode in float64.  The store-side fixes of docs/coherence.md that need no
GPU (is_current, invalidate, the one rule for C) are pinned on a toy store."""
import pytest
import torch
import torch.nn.functional as F

from tests import coherence_cases as CC

DTYPES = [torch.float32, torch.bfloat16]
UNIT = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}          # unit roundoff of one rounding to the dtype (round to nearest)


@pytest.mark.parametrize("dt", DTYPES)
def test_audit_passes_a_store_filled_from_the_definitions(dt):
    m = CC.stand_in_model(dt)
    n = CC.audit(m)
    assert n == (len(CC.STAND_IN_SHAPES) if dt == torch.bfloat16 else 0) + len(CC.STAND_IN_COPIES) + 2
    assert CC.first_stale(m) is None


def _plant(t, index, value=None):
    flat = t.view(-1)
    flat[index] = (flat[index] + 1.0) if value is None else value


PLANTS = [            # (what, copy audit must name, how to reach the tensor, flat index)
    ("C", "C[patch_embed2.proj.weight]", lambda m: m.store.C[m.store.offsets["patch_embed2.proj.weight"][0]:], 17),
    ("T", "block1.0.attn.q.weight::T", lambda m: m.store.extra["block1.0.attn.q.weight::T"], 16 * 3 + 5),
    ("T padding", "block1.0.attn.q.weight::T", lambda m: m.store.extra["block1.0.attn.q.weight::T"], 16 * 2 + 14),
    ("K", "patch_embed2.proj.weight::K", lambda m: m.store.extra["patch_embed2.proj.weight::K"], 33),
    ("KT", "patch_embed2.proj.weight::KT", lambda m: m.store.extra["patch_embed2.proj.weight::KT"], 119),
    ("K3", "t2i_head.conv4.0.weight::K", lambda m: m.store.extra["t2i_head.conv4.0.weight::K"], 1),
    ("F", "t2i_head.conv4.0.weight::F", lambda m: m.store.extra["t2i_head.conv4.0.weight::F"], 134),
    ("score W", CC.SCORE + "::W", lambda m: m.store.extra[CC.SCORE + "::W"], 20),
    ("score T", CC.SCORE + "::T", lambda m: m.store.extra[CC.SCORE + "::T"], 8 * 6 + 2),
    ("score T padding", CC.SCORE + "::T", lambda m: m.store.extra[CC.SCORE + "::T"], 8 * 4 + 7),
    ("fold weight", "fold[conv4].weight", lambda m: m._mim_fold["conv4"][1], 100),
    ("fold shift", "fold[conv4].shift", lambda m: m._mim_fold["conv4"][2], 4),
]


PLANT_CASES = [(dt, *p) for dt in DTYPES for p in PLANTS if not (p[0] == "C" and dt != torch.bfloat16)]      # (the fp32 path has no bf16 copy to plant in)


@pytest.mark.parametrize("dt,what,copy,reach,index", PLANT_CASES, ids=[f"{str(c[0]).split('.')[-1]}-{c[1]}" for c in PLANT_CASES])
def test_audit_names_a_planted_stale_element(dt, what, copy, reach, index):
    m = CC.stand_in_model(dt)
    t = reach(m)
    assert t.view(-1).numel() > index
    if "padding" in what:
        assert float(t.view(-1)[index]) == 0.0              # premise: the planted element IS a padding column
    _plant(t, index)
    assert CC.first_stale(m) == (copy, index)
    with pytest.raises(CC.StaleCopy) as e:
        CC.audit(m)
    assert e.value.copy == copy and e.value.index == index and copy in str(e.value)


def test_audit_names_the_first_of_two_and_ignores_the_gaps():
    m = CC.stand_in_model(torch.bfloat16)
    S = m.store
    off, n, _ = S.offsets["block1.0.attn.q.bias"]
    assert n % 8 and float(S.C[off + n]) == 7.0            # premise: a gap follows, and it holds the sentinel audit passed over
    S.C[off + n] = 3.0
    assert CC.first_stale(m) is None
    _plant(S.extra["patch_embed2.proj.weight::KT"], 7)
    _plant(S.extra["patch_embed2.proj.weight::K"], 9)
    assert CC.first_stale(m) == ("patch_embed2.proj.weight::K", 9)
    # a stale MASTER-side change: P moves, every copy of that parameter is stale, C is named first
    m = CC.stand_in_model(torch.bfloat16)
    m.store.master("block1.0.attn.q.weight")[2, 3] *= 2
    assert CC.first_stale(m) == ("C[block1.0.attn.q.weight]", 2 * 16 + 3)
    m = CC.stand_in_model(torch.float32)
    m.store.master("block1.0.attn.q.weight")[2, 3] *= 2
    assert CC.first_stale(m) == ("block1.0.attn.q.weight::T", 3 * 16 + 2)
    # the fold follows the BatchNorm buffers
    m = CC.stand_in_model(torch.float32)
    m.t2i_head.conv4[1].running_mean[1] += 1
    assert CC.first_stale(m) == ("fold[conv4].shift", 1)
    assert CC.first_stale(m, fold_too=False) is None
    # sign of zero and NaN are bits like any other
    m = CC.stand_in_model(torch.float32)
    m.store.extra["block1.0.attn.q.weight::T"][0, 15] = -0.0
    assert CC.first_stale(m) == ("block1.0.attn.q.weight::T", 15)
    # a copy this file has no definition for is not passed in silence
    m.store.extra["block1.0.attn.q.bias::Q"] = torch.zeros(3)
    m.store.extra["block1.0.attn.q.weight::T"][0, 15] = 0.0
    assert CC.first_stale(m) == ("block1.0.attn.q.bias::Q", -1)


# ---------------------------------------------------------------------------------------------------- the definitions against torch
def test_k_copy_is_the_weight_layout_of_an_unfolded_patch_gemm():
    """a kernel == stride conv as a GEMM over patches stored [kh][kw][cin] (the token-major gather's order): patches @ K^T == conv2d"""
    torch.manual_seed(0)
    w = torch.randn(6, 5, 2, 2, dtype=torch.float64)
    x = torch.randn(2, 5, 8, 6, dtype=torch.float64)
    want = F.conv2d(x, w, stride=2)                                                    # (2, 6, 4, 3)
    cols = F.unfold(x, 2, stride=2)                                                    # (2, cin * kh * kw, L), rows ordered [cin][kh][kw]
    patches = cols.reshape(2, 5, 2, 2, -1).permute(0, 4, 2, 3, 1).reshape(2, -1, 20)   # -> [kh][kw][cin] per patch
    got = (patches @ CC.k_copy(w).t()).permute(0, 2, 1).reshape(want.shape)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    got = (patches @ CC.kt_copy(w)).permute(0, 2, 1).reshape(want.shape)               # ::KT is the same operand, transposed
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert torch.equal(CC.kt_copy(w), CC.k_copy(w).t())
    # the 3x3, padding 1 conv through the same layout
    w3 = torch.randn(4, 3, 3, 3, dtype=torch.float64)
    x3 = torch.randn(2, 3, 5, 7, dtype=torch.float64)
    cols = F.unfold(x3, 3, padding=1).reshape(2, 3, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(2, -1, 27)
    got = (cols @ CC.k_copy(w3).t()).permute(0, 2, 1).reshape(2, 4, 5, 7)
    assert torch.allclose(got, F.conv2d(x3, w3, padding=1), rtol=0, atol=1e-12)


def test_f_copy_is_the_weight_of_the_transposed_conv():
    """the input gradient of conv3x3(pad 1) is conv_transpose2d(dz, W, padding=1): the SAME 3x3 gather over dz with the taps of ::F"""
    torch.manual_seed(1)
    w = torch.randn(4, 3, 3, 3, dtype=torch.float64)                                   # [out][cin][3][3]
    dz = torch.randn(2, 4, 5, 7, dtype=torch.float64)
    want = F.conv_transpose2d(dz, w, padding=1)                                        # (2, cin, 5, 7)
    cols = F.unfold(dz, 3, padding=1).reshape(2, 4, 3, 3, -1).permute(0, 4, 2, 3, 1).reshape(2, -1, 36)     # [dy][dx][out] per pixel
    got = (cols @ CC.f_copy(w).t()).permute(0, 2, 1).reshape(want.shape)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


def test_t_and_score_copies():
    w = torch.arange(13 * 16, dtype=torch.float32).reshape(13, 16)
    t = CC.t_copy(w)
    assert t.shape == (16, 16) and torch.equal(t[:, :13], w.t()) and not t[:, 13:].any()
    assert CC.t_copy(torch.ones(8, 3)).shape == (3, 8)                                 # a multiple of 8 gets no padding
    s = torch.arange(21, dtype=torch.float32).reshape(3, 7, 1, 1)
    assert torch.equal(CC.score_w_copy(s), s.reshape(3, 7))
    st = CC.score_t_copy(s)
    assert st.shape == (7, 8) and torch.equal(st[:, :3], s.reshape(3, 7).t()) and not st[:, 3:].any()


@pytest.mark.parametrize("dt", DTYPES)
def test_fold_is_eval_batchnorm_behind_the_conv(dt):
    """(W', b') against F.batch_norm(F.conv2d(x, W)) on the running statistics in float64.  W' is ONE rounding of the exact product to the operand dtype (plus
    the fp32 arithmetic that forms it: two roundings in the scale, one in the product -- 3 fp32 units), b' three fp32 roundings of values up to
    |beta| + |mean * scale|; the output bound is those errors carried through the conv's sum of |x| |W'|."""
    torch.manual_seed(2)
    cout, cin = 5, 3
    w = torch.randn(cout, cin, 3, 3)
    gamma, beta = torch.rand(cout) + 0.5, torch.randn(cout)
    mean, var = torch.randn(cout), torch.rand(cout) + 0.1
    x = torch.randn(2, cin, 6, 5, dtype=torch.float64)
    wk, shift = CC.fold(w, gamma, beta, mean, var, dt)
    assert wk.dtype == dt and wk.shape == (cout, 9 * cin) and shift.dtype == torch.float32
    d = lambda t: t.double()
    scale64 = d(gamma) / torch.sqrt(d(var) + CC.BN_EPS)
    w64 = CC.k_copy(d(w)) * scale64[:, None]
    u = UNIT[dt] + 4 * UNIT[torch.float32]
    assert bool(((d(wk) - w64).abs() <= u * w64.abs()).all())
    b64 = d(beta) - d(mean) * scale64
    assert bool(((d(shift) - b64).abs() <= 4 * UNIT[torch.float32] * (d(beta).abs() + (d(mean) * scale64).abs())).all())
    want = F.batch_norm(F.conv2d(x, d(w), padding=1), d(mean), d(var), d(gamma), d(beta), False, 0.1, CC.BN_EPS)
    w_back = d(wk).reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)                        # ::K order back to [out][cin][3][3]
    got = F.conv2d(x, w_back, padding=1) + d(shift)[None, :, None, None]
    bound = u * F.conv2d(x.abs(), w_back.abs(), padding=1) * (1 + 2 * u) + (4 * UNIT[torch.float32] * (d(beta).abs() + (d(mean) * scale64).abs()))[None, :, None, None] + 1e-13
    assert bool(((got - want).abs() <= bound).all()), float(((got - want).abs() / bound).max())
    if dt == torch.bfloat16:      # the rounding is really ONE: rounding the fp32 product again changes nothing, rounding W first and then scaling does
        assert torch.equal(wk, (CC.k_copy(w) * (gamma * torch.rsqrt(var + CC.BN_EPS))[:, None]).to(dt))
        twice = (CC.k_copy(w.to(dt)).float() * (gamma * torch.rsqrt(var + CC.BN_EPS))[:, None]).to(dt)
        assert not torch.equal(wk, twice)


# ---------------------------------------------------------------------------------------------------- the store, on a toy model
def _toy():
    import torch.nn as nn
    from mvlt_amd.params import FlatStore, Holder

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.first = Holder(weight=(5, 3))
            self.mid = nn.ModuleList([Holder(weight=(4, 4), bias=(4,)), Holder(weight=(3, 7))])
            self.head = Holder(weight=(2, 6), bias=(2,))
            self.tied = nn.Module()
            self.tied.weight = self.first.weight
            self.last = Holder(weight=(9,))
            for i, p in enumerate(self.parameters()):
                nn.init.constant_(p, float(i + 1))
            self.store = None

    m = Toy()
    S = FlatStore(m, torch.float32)
    object.__setattr__(m, "store", S)
    S.materialize(torch.device("cpu"))
    return m, S


def test_is_current_notices_a_replacement_anywhere_in_the_model():
    """hypothesis 2 of docs/coherence.md: the first and the last parameter say nothing about the middle"""
    from mvlt_amd.params import Holder
    m, S = _toy()
    assert S.is_current() and len(S.params) == 7
    assert len(S._param_slots) == 8                                     # the tied weight has two slots, one offset
    m.head = Holder(weight=(2, 6), bias=(2,))                           # a whole child module
    assert not S.is_current()
    with torch.no_grad():
        m.head.weight.fill_(0.5)
    S.ensure(torch.device("cpu"))
    assert S.is_current() and S.params["head.weight"] is m.head.weight and float(S.master("head.weight")[1, 2]) == 0.5
    assert float(S.master("mid.1.weight")[0, 0]) == 4.0 and float(S.master("last.weight")[0]) == 7.0      # the others kept their values
    m.mid[0].weight.data = torch.full((4, 4), 9.0)                      # p.data = other, in the middle
    assert not S.is_current()
    S.ensure(torch.device("cpu"))
    assert S.is_current() and float(S.master("mid.0.weight")[3, 3]) == 9.0
    m.mid[1].weight = torch.nn.Parameter(torch.full((3, 7), 2.5))       # a new Parameter in an old module
    assert not S.is_current()
    S.ensure(torch.device("cpu"))
    assert S.is_current() and float(S.master("mid.1.weight")[2, 6]) == 2.5
    m.tied.weight = torch.nn.Parameter(torch.zeros(5, 3))               # un-tying: the second slot of the tied weight
    assert not S.is_current()
    S.ensure(torch.device("cpu"))
    assert S.is_current() and len(S.params) == 8
    P = S.P
    S.ensure(torch.device("cpu"))
    assert S.P is P                                                     # nothing replaced: nothing rebuilt


def test_invalidate_and_the_one_rule_for_the_bf16_copy():
    """hypotheses 1 and 3 on the host side: what the fused writers ask before and declare after their launch"""
    m, S = _toy()
    S.C = torch.zeros(S.total, dtype=torch.bfloat16)                    # (a bf16 store on the CPU: the flags alone are under test)
    assert not S.c_is_current()                                         # just materialised: C is uninitialised
    S._cast_version, S.force_dirty = S.versions(), False                # what refresh() leaves
    assert S.c_is_current()
    S.c_written_by_kernel(True, wrote_all=False)                        # a frozen / gated step on a current copy
    assert S.force_dirty and S._c_fresh_version == S.versions() and S.c_is_current()
    with torch.no_grad():
        m.head.weight.mul_(2)                                           # someone writes the parameters ...
    assert not S.c_is_current()
    S.c_written_by_kernel(S.c_is_current(), wrote_all=False)            # ... and the kernel skips elements: C is NOT declared fresh
    assert S._c_fresh_version is None and S.force_dirty
    S.c_written_by_kernel(False, wrote_all=True)                        # it wrote every element: fresh whatever was before
    assert S._c_fresh_version == S.versions()
    v = S.versions()
    m.head.weight.data.mul_(2)                                          # the invisible writer
    assert S.versions() == v and S.c_is_current()                       # (the premise of invalidate(): nothing noticed)
    S.invalidate()
    assert S.force_dirty and S._c_fresh_version is None and S._cast_version == -1 and not S.c_is_current()
    S.C = None
    assert not S.c_is_current()
    S.c_written_by_kernel(False, wrote_all=True)
    assert S._c_fresh_version is None                                   # the fp32 path has no copy to declare


def test_fused_adamw_refuses_a_parameter_it_was_not_built_with():
    from mvlt_amd.optim import FusedAdamW
    from mvlt_amd.params import Holder
    m, S = _toy()
    opt = FusedAdamW(m, lr=1e-3)
    opt._ensure()
    m.mid[0].weight.data = torch.full((4, 4), 9.0)                      # same Parameter, new storage: the optimizer follows the re-materialised store
    S.ensure(torch.device("cpu"))
    opt._ensure()
    assert opt._mask_key[0] == S.P.data_ptr()
    m.head = Holder(weight=(2, 6), bias=(2,))
    S.ensure(torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"head\.weight.*replaced"):
        opt._ensure()
