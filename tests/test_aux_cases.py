# CPU-only checks of the exact tests of the auxiliary kernels
# (tests/_aux_cases.py, used by test_gpu_aux_exact.py): the gemv and sum
# references are exact (recomputed in int64 from the numerators), so the
# bit-equality bars of the GPU module are sound; every table entry
# satisfies the argument contract of its entry (the Python restatement
# that test_aux_guards.py compares with the header); and the tables reach
# the edges they name.
import numpy as np
import pytest

import _aux_cases as AC
import _exact
from _exact import dtype_of

QB = _exact.F64_QBITS


@pytest.mark.parametrize("m,n,lda", AC.GEMV_SHAPES)
def test_gemv_reference_is_exact(m, n, lda):
    a, x, qa, qx, ref = AC.gemv_inputs(m, n)
    assert n <= _exact.F64_KMAX and qa.dtype == qx.dtype == np.int64
    assert np.abs(qa).max() <= _exact.F64_QMAX >= np.abs(qx).max()
    np.testing.assert_array_equal(a, qa * 2.0 ** -QB)
    np.testing.assert_array_equal(x, qx * 2.0 ** -QB)
    # any order of partial sums stays below 2^53 units of 2^-38
    assert (np.abs(qa) @ np.abs(qx)).max() < 2 ** 53
    exact = qa @ qx                                   # int64, cannot overflow
    np.testing.assert_array_equal(ref, exact.astype(np.float64) * 2.0 ** (-2 * QB))
    # no zero in the expected vector: its sign is not in question
    assert (ref != 0).all()


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("n", AC.SUM_NS)
def test_sum_reference_is_exact(n, fp32):
    vals, q, expected = AC.sum_inputs(n, fp32)
    assert vals.dtype == dtype_of(fp32) and vals.shape == (n,)
    assert n <= 2 ** 20
    amax = _exact.F32_AMAX if fp32 else _exact.F64_QMAX
    assert np.abs(q).max() <= amax
    # worst partial sum in any order: n * amax units, far below 2^53
    assert n * amax < 2 ** 40
    scale = 1.0 if fp32 else 2.0 ** -QB
    np.testing.assert_array_equal(vals.astype(np.float64), q * scale)
    total = int(q.sum())                              # int64, cannot overflow
    assert expected == total * scale
    assert float(total) == total


def test_sum_sizes_straddle_block_and_grid():
    assert {255, 256, 257} <= set(AC.SUM_NS)
    grid = 1024 * 256
    assert {grid - 1, grid, grid + 1} <= set(AC.SUM_NS)
    assert max(AC.SUM_NS) > 2 * grid


def test_gemv_shapes_reach_the_named_edges():
    def chunks(n):
        clen = -(-n // 32)
        return [max(0, min(n, (c + 1) * clen) - c * clen) for c in range(32)]
    by = {(m, n): chunks(n) for m, n, _ in AC.GEMV_SHAPES}
    assert by[(5, 31)] == [1] * 31 + [0]
    assert by[(257, 33)][:17] == [2] * 16 + [1] and not any(by[(257, 33)][17:])
    assert 16 * 2 + 2 > 33                      # chunks from 17 on start past n
    assert set(by[(256, 128)]) == {4}
    assert by[(300, 200)][0] == 7 and 7 % 4 == 3
    live = [c for c in by[(513, 161)] if c]
    assert live[-1] == 5 and live[0] == 6        # last live chunk: 1-col tail
    assert by[(64, 4096)][0] == 128
    assert {c % 4 for v in by.values() for c in v if c} == {0, 1, 2, 3}
    assert any(m % 256 == 1 and m > 256 for m, _, _ in AC.GEMV_SHAPES)
    assert any(lda > m for m, _, lda in AC.GEMV_SHAPES)
    for m, n, lda in AC.GEMV_SHAPES:
        img = AC.gemv_device_image(m, n, lda)
        assert img.shape == (lda, n + 1)
        assert np.isnan(img[m:, :]).all() and np.isnan(img[:, n:]).all()
        assert not np.isnan(img[:m, :n]).any()


def test_tables_satisfy_the_entry_contracts():
    for m, n, lda in AC.GEMV_SHAPES:
        assert AC.gemv_ok(lda * (n + 1) * 8, m, n, lda)
    for fp32 in (0, 1):
        e = AC.elem_of(fp32)
        for m, n in AC.TRANSPOSE_SHAPES:
            nbytes = (m * n + AC.TAIL) * e
            assert AC.transpose_ok(fp32, m, n, nbytes, nbytes)
        for n in AC.FILL_NS:
            assert AC.fill_ok((n + AC.TAIL) * e, fp32, n)
        for rt, ct, ld, m, n in AC.ZERO_PAD_CASES:
            assert AC.zero_pad_ok(ld * (ct + 1) * e, fp32, rt, ct, ld, m, n)
    from marlin_amd.engine import Engine
    assert sorted(Engine.OPS) == sorted(AC.MAP_OPS)
    for op in Engine.OPS.values():
        assert AC.map_op_ok(op)


def test_fill_and_zero_pad_tables_pass_one_grid():
    grid = 2048 * 256
    assert {grid, grid + 1} <= set(AC.FILL_NS) and max(AC.FILL_NS) > 2 * grid
    assert 2 ** 64 - 1 in AC.FILL_SEEDS and 0 in AC.FILL_SEEDS
    assert any(rt * ct > grid for rt, ct, _, _, _ in AC.ZERO_PAD_CASES)
    assert any(ld > rt for rt, _, ld, _, _ in AC.ZERO_PAD_CASES)
    assert any(m == 0 for *_, m, _ in AC.ZERO_PAD_CASES)
    assert any(n == 0 for *_, n in AC.ZERO_PAD_CASES)


@pytest.mark.parametrize("fp32", [0, 1])
def test_fill_expected_is_the_rounded_double_stream(fp32):
    v64 = AC.fill_expected(1000, 2 ** 64 - 1, 0)
    v = AC.fill_expected(1000, 2 ** 64 - 1, fp32)
    np.testing.assert_array_equal(v, v64.astype(dtype_of(fp32)))
    assert (v64 >= 0).all() and (v64 < 1).all()
    assert (AC.fill_expected(1000, 0, 0) != v64).any()


@pytest.mark.parametrize("fp32", [0, 1])
def test_zero_pad_images(fp32):
    for case in AC.ZERO_PAD_CASES:
        rt, ct, ld, m, n = case
        img, want = AC.zero_pad_images(case, fp32)
        assert img.shape == (ld, ct + 1) and (img != 0).all()
        changed = AC.bits(img) != AC.bits(want)
        pad = np.zeros(img.shape, dtype=bool)
        pad[m:rt, :ct] = True
        pad[:rt, n:ct] = True
        np.testing.assert_array_equal(changed, pad)
        assert (AC.bits(want)[pad] == 0).all()                 # +0, not -0
    # a kernel that indexed its stores with rows_total where the pitch is
    # due writes other elements wherever ld > rows_total
    rt, ct, ld, m, n = AC.ZERO_PAD_CASES[1]
    img, want = AC.zero_pad_images(AC.ZERO_PAD_CASES[1], fp32)
    wrong = img.copy(order="F").reshape(-1, order="F")
    for c in range(ct):
        for r in range(rt):
            if r >= m or c >= n:
                wrong[c * rt + r] = 0
    assert (wrong.reshape(img.shape, order="F") != want).any()


@pytest.mark.parametrize("fp32", [0, 1])
def test_transpose_inputs_carry_the_payloads(fp32):
    dt = dtype_of(fp32)
    for m, n in AC.TRANSPOSE_SHAPES:
        a = AC.transpose_input(m, n, fp32)
        assert a.shape == (m, n) and a.dtype == dt and a.flags.f_contiguous
        b = AC.bits(a.reshape(-1, order="F"))
        assert b[0] == AC.PAYLOAD_BITS[dt] and np.isnan(a[0, 0])
        if a.size >= 3:
            assert AC.NEG_ZERO_BITS[dt] in b and AC.SUBNORMAL_BITS[dt] in b
            assert AC.is_subnormal(a).sum() == 1
    shapes = set(AC.TRANSPOSE_SHAPES)
    assert {(1, 1), (32, 32), (31, 33), (33, 31)} <= shapes
    assert any(m == 1 and n > 32 for m, n in shapes)
    assert any(n == 1 and m > 32 for m, n in shapes)


@pytest.mark.parametrize("fp32", [0, 1])
def test_map_inputs_hold_every_pair_of_specials(fp32):
    s = AC.map_specials(fp32)
    a, b = AC.map_inputs(fp32)
    assert a.size == b.size == 64 and a.dtype == b.dtype == dtype_of(fp32)
    pairs = {(int(x), int(y)) for x, y in zip(AC.bits(a), AC.bits(b))}
    assert len(pairs) == 64
    assert np.isnan(s[0]) and np.isposinf(s[1]) and np.isneginf(s[2])
    assert s[3] == 0 and not np.signbit(s[3]) and np.signbit(s[4])
    assert s[5] == np.finfo(s.dtype).max and s[6] == np.finfo(s.dtype).tiny
    assert AC.is_subnormal(s).tolist() == [False] * 7 + [True]
    # the lanes the division tests leave out: at most three of the eight
    # values of a (subnormal, smallest normal, largest finite), 8 lanes each
    for op in ("divs", "rdivs"):
        for name in AC.MAP_SCALARS:
            sc = AC.map_scalar(name, fp32)
            want = AC.map_expected(op, a, None, sc)
            out = AC.is_subnormal(a) | AC.is_subnormal(want)
            assert out.sum() <= 24
            assert set(np.flatnonzero(out) // 8) <= {5, 6, 7}
