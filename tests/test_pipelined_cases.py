# CPU-only checks of the case tables of test_gpu_gemm_pipelined.py: every
# K stays inside the bounds tests/_exact.py proves exact, ids are unique,
# and the tables hold the tile counts and fallbacks they are there for.
import _exact
import _pipelined_cases as PC


def test_exact_tables_within_proven_bounds_and_unique():
    for variant in PC.VARIANTS:
        cases = PC.exact_cases(variant)
        ids = [_exact.case_id(c) for c in cases]
        assert len(set(ids)) == len(ids) == len(set(cases))
        for c in cases:
            assert c.K <= (_exact.F32_KMAX if c.fp32 else _exact.F64_KMAX)
            assert c.M % 128 == 0 and c.N % 128 == 0 and c.K % 32 == 0
        assert {(c.fp32, c.beta) for c in cases} \
            == {(f, b) for f in (0, 1) for b in (0, 1)}


def test_exact_tables_hold_the_intended_tile_counts():
    base = PC.exact_cases("base")
    assert {c.K // 16 for c in base if not c.fp32} == {4, 256}
    assert {c.K // 16 for c in base if c.fp32} == {4, 32}
    for variant in ("bk32", "bm256", "phase1", "phase8"):
        cases = PC.exact_cases(variant)
        assert {c.K for c in cases if not c.fp32} == {_exact.F64_KMAX}
        assert {c.K for c in cases if c.fp32} == {_exact.F32_KMAX}
        assert {c.M for c in cases} == {384, 512}
    # bm256: 512 rows select the 256-row tile, 384 rows and fp32 fall back
    env = PC.VARIANTS["bm256"]
    bms = {(c.fp32, c.M): _exact.expected_config(env, c)["bm"]
           for c in PC.exact_cases("bm256")}
    assert bms == {(0, 384): 128, (0, 512): 256, (1, 384): 128, (1, 512): 128}
    env = PC.VARIANTS["bk32"]
    assert {_exact.expected_config(env, c)["bk"]
            for c in PC.exact_cases("bk32")} == {32}


def test_loop_and_bits_tables():
    assert PC.LOOPS == {"default": {}, "twobar": {PC.LOOP_KNOB: "twobar"},
                        "pipe": {PC.LOOP_KNOB: "pipe"}}
    assert PC.LOOP_KNOB in PC.KNOBS
    for fp32 in (0, 1):
        for bk in (16, 32):
            cfg = {"is_fp32": fp32, "bk": bk}
            assert PC.expected_loop("twobar", cfg) == 0
            assert PC.expected_loop("pipe", cfg) == 1
            # per-variant default: only fp32 at BK=16 keeps two barriers
            assert PC.expected_loop("default", cfg) == (0 if (fp32, bk) == (1, 16) else 1)
    m, n, k = PC.BITS_SHAPE
    assert m % 128 == 0 and n % 128 == 0 and k % 16 == 0
    assert (k // 16) % 2 == 1 and m // 128 > 1 and n // 128 > 1
    ids = [PC.bits_id(*c) for c in PC.BITS_CASES]
    assert len(set(ids)) == len(ids) == 4
    assert len(set(PC.BITS_SEEDS)) == 3
