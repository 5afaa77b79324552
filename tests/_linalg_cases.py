# Inputs for the decomposition tier (marlin_amd/linalg.py) on which the
# block-local pivoting of lu_decompose has something to do, and a numpy
# stand-in for the engine so that the permutation logic runs on any
# machine. Shared by test_linalg_cpu.py, test_gpu_linalg.py and
# test_gpu_grouped_consumers.py.
import numpy as np

from marlin_amd.linalg import _split
from oracle import gen_matrix


def shuffled_dominant(n, base, seed=None):
    """(a, src): a diagonally dominant matrix d with its rows shuffled
    inside each block row of _split(n, base) by a fixed-seed permutation;
    row g of a is row src[g] of d. Partial pivoting inside a diagonal block
    then has to undo the shuffle: src[p_array] == arange(n)."""
    seed = 0x5A0F + 31 * n + base if seed is None else seed
    d = gen_matrix(n, n, seed=seed) + n * np.eye(n)
    _, offs, lens = _split(n, base)
    rng = np.random.RandomState(seed % 2 ** 32)
    src = np.arange(n)
    for o, ln in zip(offs, lens):
        src[o:o + ln] = o + rng.permutation(ln)
    return np.asfortranarray(d[src, :]), src


def lu_residual(a, lu, p_array):
    """max|P A - L U| / max|A| for the packed L\\U of lu_decompose."""
    n = a.shape[0]
    L = np.tril(lu, -1) + np.eye(n)
    return np.max(np.abs(a[p_array, :] - L @ np.triu(lu))) / np.max(np.abs(a))


class HostMatrix:
    """What the stand-in hands out where the engine hands out a
    DeviceMatrix."""

    def __init__(self, a):
        self.a = np.array(a, dtype=np.float64, order="F")
        self.m, self.n = self.a.shape
        self.fp32 = False
        self.freed = False

    def free(self):
        assert not self.freed, "freed twice"
        self.freed = True


class NumpyEngine:
    """The part of Engine that linalg.py uses, in numpy float64."""

    def __init__(self):
        self.grouped_calls = 0
        self.live = []

    def upload_matrix(self, a, fp32=False):
        assert not fp32
        h = HostMatrix(a)
        self.live.append(h)
        return h

    def download_matrix(self, dm):
        assert not dm.freed
        return dm.a.copy(order="F")

    def gemm_dd(self, A, B, C=None, accumulate=False, trans_a=False,
                trans_b=False, split_k=None):
        assert not (A.freed or B.freed)
        prod = (A.a.T if trans_a else A.a) @ (B.a.T if trans_b else B.a)
        if C is None:
            assert not accumulate
            return self.upload_matrix(prod)
        assert not C.freed and C.a.shape == prod.shape
        C.a[...] = C.a + prod if accumulate else prod
        return C

    def gemm_grouped(self, problems, accumulate=False, trans_a=False,
                     trans_b=False):
        self.grouped_calls += 1
        # independent products: no C of the batch is an operand of it
        cs = [id(C) for _, _, C in problems if C is not None]
        assert len(set(cs)) == len(cs)
        assert not {id(x) for A, B, _ in problems for x in (A, B)} & set(cs)
        return [self.gemm_dd(A, B, C, accumulate=accumulate, trans_a=trans_a,
                             trans_b=trans_b) for A, B, C in problems]
