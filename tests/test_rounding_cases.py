# CPU self-test of the rounding checker (tests/_rounding_cases.py): the
# criteria the GPU test holds the kernels to accept correct round-to-nearest
# arithmetic in three summation orders, on every data class, and each
# degraded model is rejected by the criterion meant for it. This is the proof,
# without a GPU, that test_gpu_gemm_rounding.py can fail.
import numpy as np
import pytest

import _rounding_cases as RC
from _rounding_cases import KS, M, N

TYPES = [0, 1]
_TID = ["f64", "f32"]
CHAINS = {"sequential": RC.chain_sequential, "group4": RC.chain_group4,
          "pairwise": RC.chain_pairwise}


def _accepts(got, r, s, fp32, terms, cls):
    return RC.failures(RC.measure(got, r, s, fp32, terms), RC.criteria(cls))


def _rejected_by(got, r, s, fp32, terms, criterion):
    """The criterion fails on `got` (the figures go into the message)."""
    mes = RC.measure(got, r, s, fp32, terms)
    assert RC.failures(mes, (criterion,)), \
        f"{criterion} accepted a degraded result: {mes}"
    return mes


# ---------------------------------------------------------------------------
# accepted: correct chains
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cls", RC.CLASSES)
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_correct_chains_are_accepted(fp32, cls, k):
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    for name, chain in CHAINS.items():
        bad = _accepts(chain(a, b), r, s, fp32, k, cls)
        assert not bad, f"{name}: {bad}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cls", ["pos", "mix", "wide"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_correct_chains_with_addend_are_accepted(fp32, cls, k):
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    c0 = RC.operand(cls, "c", fp32, M, N)
    r1, s1 = RC.with_addend(r, s, c0, fp32)
    for name, chain in CHAINS.items():
        bad = _accepts(chain(a, b, c0), r1, s1, fp32, k + 1, cls)
        assert not bad, f"{name}: {bad}"


# ---------------------------------------------------------------------------
# rejected: the degraded models
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cls", ["pos", "mix"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_ten_bit_inputs_fail_the_hard_bound(fp32, cls, k):
    # model (a): tf32-like operands, everything else correct
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    got = RC.chain_sequential(RC.cut_mantissa(a, 10), RC.cut_mantissa(b, 10))
    _rejected_by(got, r, s, fp32, k, "H")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_inputs_short_of_three_bits_fail_the_bias_criterion(fp32, k):
    # model (b): fp32 operands cut to 20 mantissa bits (fp64: to 49, the
    # same three bits short). Inside the hard bound, which is why S2 exists.
    a, b, r, s = RC.product("pos", fp32, M, k, N)
    keep = np.finfo(a.dtype).nmant - 3
    got = RC.chain_sequential(RC.cut_mantissa(a, keep),
                              RC.cut_mantissa(b, keep))
    mes = _rejected_by(got, r, s, fp32, k, "S2")
    assert not RC.failures(mes, ("H",)), "model (b) is meant to pass H"
    if k <= 64:
        assert RC.failures(mes, ("S1",)), f"S1 accepted model (b): {mes}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_round_toward_zero_fails_the_statistics(fp32, k):
    # model (c): inside the hard bound as well; biased, so the mean and
    # the rms of t grow like k instead of sqrt(k)
    a, b, r, s = RC.product("pos", fp32, M, k, N)
    got = RC.chain_toward_zero(a, b)
    mes = _rejected_by(got, r, s, fp32, k, "S2")
    assert not RC.failures(mes, ("H",)), "model (c) is meant to pass H"
    assert RC.failures(mes, ("S1",)), f"S1 accepted model (c): {mes}"


@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_flushed_subnormals_fail_the_hard_bound(fp32, k):
    # model (d)
    a, b, r, s = RC.product("sub_out", fp32, M, k, N)
    got = RC.flush_subnormal(RC.chain_sequential(a, b))
    mes = _rejected_by(got, r, s, fp32, k, "H")
    assert mes["h"] > 100


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cls", ["pos", "mix"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_one_moved_element_fails_the_hard_bound(fp32, cls, k):
    # model (e): the bound is componentwise, one element is enough
    _, _, r, s = RC.product(cls, fp32, M, k, N)
    at = (M // 2, N // 3)
    mes = _rejected_by(RC.move_one(r, s, fp32, k, at), r, s, fp32, k, "H")
    assert mes["bad"] == 1 and mes["first_bad"] == list(at)
    # and the very same result without the move is accepted
    assert not _accepts(r.astype(RC.dtype_of(fp32)), r, s, fp32, k, cls)


def test_not_finite_results_fail_the_hard_bound():
    a, b, r, s = RC.product("mix", 1, M, 16, N)
    for v in (np.nan, np.inf):
        got = RC.chain_sequential(a, b)
        got[3, 5] = v
        mes = _rejected_by(got, r, s, 1, 16, "H")
        assert mes["first_bad"] == [3, 5]


def test_zero_scale_demands_an_exact_zero():
    a, b, _, _ = RC.product("mix", 0, M, 16, N)
    a = np.array(a)
    a[7, :] = 0
    rt = RC.ref_type(0)
    r = a.astype(rt) @ b.astype(rt)
    s = np.abs(a).astype(rt) @ np.abs(b).astype(rt)
    got = RC.chain_sequential(a, b)
    assert RC.measure(got, r, s, 0, 16)["zero_ok"]
    got[7, 9] = 2.0 ** -1074              # inside H's underflow allowance
    mes = RC.measure(got, r, s, 0, 16)
    assert not mes["zero_ok"] and RC.failures(mes, ("H",))


# ---------------------------------------------------------------------------
# the data classes are what they say
@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_sub_out_results_are_all_subnormal(fp32, k):
    a, b, r, _ = RC.product("sub_out", fp32, M, k, N)
    tiny = RC.tiny(fp32)
    assert (np.abs(a) >= tiny).all() and (np.abs(b) >= tiny).all()
    assert ((np.abs(r) > 0) & (np.abs(r) < tiny)).all()
    got = RC.chain_sequential(a, b)
    assert (np.abs(got) < tiny).all()
    assert np.count_nonzero(got) >= got.size - 16
    # every single product is subnormal too
    rt = RC.ref_type(fp32)
    assert np.abs(a).max().astype(rt) * np.abs(b).max().astype(rt) < tiny


@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_sub_in_inputs_are_subnormal_and_results_normal(fp32, k):
    a, b, r, _ = RC.product("sub_in", fp32, M, k, N)
    tiny = RC.tiny(fp32)
    assert (np.abs(a) < tiny).all() and np.count_nonzero(a) == a.size
    assert (np.abs(b) >= tiny).all()
    got = RC.chain_sequential(a, b)
    assert (np.abs(got) >= tiny).all() and (np.abs(r) >= tiny).all()


@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_inputs_are_rounded_before_the_reference_sees_them(fp32):
    dt = RC.dtype_of(fp32)
    for cls in RC.CLASSES:
        a, b, r, s = RC.product(cls, fp32, M, 16, N)
        assert a.dtype == b.dtype == dt
        assert r.dtype == s.dtype == RC.ref_type(fp32)
        assert not (a.flags.writeable or r.flags.writeable)
    assert RC.product("mix", fp32, M, 16, N)[2] is \
        RC.product("mix", fp32, M, 16, N)[2]          # cached
    mix = RC.operand("mix", "a", fp32, M, 64)
    assert (mix < 0).any() and (mix > 0).any()
    wide = RC.operand("wide", "a", fp32, M, 64)
    e = np.frexp(wide.astype(np.float64))[1]
    assert e.min() < -15 and e.max() > 15


def test_variant_tables():
    for v in RC.VARIANTS:
        cases = RC.variant_cases(v)
        assert len({RC.variant_case_id(c) for c in cases}) == len(cases)
        for (fp32, beta, cls, m, n, k) in cases:
            assert m <= 256 and n <= 256 and k <= 1056
            assert not (beta and cls == "sub_out")
    assert {c[5] for c in RC.variant_cases("bk32")} == {32, 288, 1056}
    assert {(c[0], c[3]) for c in RC.variant_cases("bm256")} == {(0, 256)}
