"""The NumPy statement of the GEMM's contract (tests/gemm_reference.py) against triple loops in Python integers, at sizes a
loop can do and with a block size of 4 or 6 in place of 128, so that 20 x 20 operands reach every K-range and triangle rule.
The loops follow the KERNEL's definition -- a tile's K range, tile by tile -- and refuse to touch poison; the module under
test states the same product as one matmul of masked operands.  No GPU."""
import itertools

import numpy as np
import pytest

import gemm_reference as gr


def _tile_k_range(s, m0, n0, t):
    """K range of the t-wide tile at (m0, n0): the rules of dgemm.hip's K-range modes"""
    K, km = s["K"], s["kmode"]
    kbeg, kend = 0, K
    if km == 1:
        kbeg, kend = m0, min(m0 + t, K)
    elif km == 2:
        kbeg, kend = n0, min(n0 + t, K)
    elif km == 3:
        kend = min(m0 + t, K)
    elif km == 4:
        kend = min(n0 + t, K)
    elif km == 7:
        kbeg, kend = n0, min(m0 + t, K)
    return kbeg, kend


def _loop_product(s, A, B, C0, t, part=None):
    """exact C [batch][M][N] as Python numbers, every element summed over the K range of the t-wide tile it lies in, read
    from the flat buffers by address arithmetic.  Halves are kept exact by working in units of 1/8."""
    M, N, K = s["M"], s["N"], s["K"]
    a8, b8 = int(s["alpha"] * 8), int(s["beta"] * 8)
    assert a8 == s["alpha"] * 8 and b8 == s["beta"] * 8
    cidx = gr.c_index(s)
    out = [[[None] * N for _ in range(M)] for _ in range(s["batch"])]
    for b, r, c in itertools.product(range(s["batch"]), range(M), range(N)):
        kbeg, kend = _tile_k_range(s, r // t * t, c // t * t, t)
        acc = 0
        for k in range(kbeg, kend):
            av = A[s["a_off"] + b * s["bsa"] + (k * s["lda"] + r if s["ta"] else r * s["lda"] + k)]
            bv = B[s["b_off"] + b * s["bsb"] + (c * s["ldb"] + k if s["tb"] else k * s["ldb"] + c)]
            assert av == av and bv == bv, f"poison inside the K range of tile size {t} at (r, c, k) = {(r, c, k)}"
            assert av == int(av) and bv == int(bv)
            acc += int(av) * int(bv)
        v = a8 * acc
        if s["beta"] != 0.0 and s["split_k"] <= 1:
            c0 = C0[cidx[b, r, c]]
            assert c0 == int(c0)
            v += b8 * int(c0)
        out[b][r][c] = v / 8.0
    return np.array(out)


def _small(M, N, K, **kw):
    return gr.make_spec(M, N, K, **kw)


SMALL = ([_small(M, N, K, align=al, ta=ta, tb=tb, alpha=0.5, beta=-2.0)
          for (M, N, K) in [(1, 1, 1), (7, 20, 5), (19, 6, 13)] for (ta, tb) in gr.LAYOUTS for al in gr.ALIGNS] +
         [_small(17, 17, 17, ta=ta, tb=tb, kmode=km, lower_only=lo, alpha=-1.0, beta=b)
          for km in (1, 2) for lo in (0, 1, 2, 3) for (ta, tb) in gr.LAYOUTS for b in (0.0, 1.0)] +
         [_small(19, 11, 19, ta=ta, tb=tb, kmode=3) for (ta, tb) in gr.LAYOUTS] +
         [_small(11, 19, 19, ta=ta, tb=tb, kmode=4, alpha=2.0) for (ta, tb) in gr.LAYOUTS] +
         [_small(m, m, m, ta=ta, tb=tb, kmode=7, lower_only=1, alpha=0.5, beta=-2.0) for m in (12, 19) for (ta, tb) in gr.LAYOUTS] +
         [_small(9, 8, 6, batch=3, ta=1, alpha=0.5, beta=-2.0), _small(14, 9, 9, tb=1, kmode=2, c_in_a_col=0),
          _small(5, 13, 12, c_in_b_off=7 * _small(5, 13, 12)["ldb"])])


@pytest.mark.parametrize("blk", [4, 6])
@pytest.mark.parametrize("i", range(len(SMALL)))
def test_expected_against_integer_loops(i, blk):
    s = SMALL[i]
    rng = np.random.default_rng(1000 + i)
    for poison in (True, False):
        A, B, C0 = gr.make_operands(s, rng, poison=poison, blk=blk)
        assert A.size == gr.buffer_sizes(s)[0] and B.size == gr.buffer_sizes(s)[1]
        held = A if s["c_in_a_col"] >= 0 else (B if s["c_in_b_off"] >= 0 else C0)
        exp = gr.expected(s, A, B, held, blk=blk)
        # the kernel runs blk-wide tiles or blk / 2-wide ones (the block-diagonal modes: blk only): one product either way
        for t in ([blk] if s["kmode"] in (1, 2) else [blk, blk // 2]):
            assert np.array_equal(exp, _loop_product(s, A, B, held, t)), (s, t)
        if poison:      # everything outside the logical operands is poison, and so is what no tile's K range reaches
            uA, uB, _, _ = gr.used(s, blk)
            assert np.isnan(A).sum() == A.size - s["batch"] * int(uA.sum())
            assert np.isnan(B).sum() == B.size - s["batch"] * int(uB.sum())
            if C0 is not None:
                assert np.isnan(C0).sum() == C0.size - (s["batch"] * s["M"] * s["N"] if s["beta"] != 0.0 else 0)


@pytest.mark.parametrize("blk", [4, 6])
@pytest.mark.parametrize("lo", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(17, 17), (20, 9), (9, 20), (1, 1)])
def test_masks_against_loops(shape, lo, blk):
    M, N = shape
    for s in (gr.make_spec(M, N, 3, lower_only=lo), gr.make_spec(M, N, 3, lower_only=lo, batch=2),
              gr.make_spec(M, N, 3, lower_only=lo, split_k=3)):
        size = gr.buffer_sizes(s)[2]
        req, forb, eith = gr.masks(s, size, blk)
        want = np.full(size, "f")
        for b, p, r, c in itertools.product(range(s["batch"]), range(s["split_k"]), range(M), range(N)):
            i = s["c_off"] + b * s["bsc"] + p * M * s["ldc"] + r * s["ldc"] + c
            tr, tc = r // blk, c // blk
            if lo == 0:
                want[i] = "r"
            elif lo == 1:
                want[i] = "r" if c <= r else ("f" if tc > tr else "e")
            elif lo == 2:
                want[i] = "r" if tc < tr else ("f" if tc > tr else "e")
            else:
                want[i] = "r" if c >= r else ("f" if tc < tr else "e")
        assert np.array_equal(req, want == "r") and np.array_equal(forb, want == "f") and np.array_equal(eith, want == "e")
        # a blk / 2-wide tiling writes a subset of what a blk-wide one writes, and both write everything required
        for t in (blk, blk // 2):
            tr, tc = np.arange(M)[:, None] // t, np.arange(N)[None, :] // t
            written = {0: tr * 0 + tc * 0 == 0, 1: tc <= tr, 2: tc < tr, 3: tc >= tr}[lo]
            idx = gr.c_index(s)
            assert not (req[idx][0] & ~written).any() and not (forb[idx][0] & written).any()


def test_in_place_masks_cover_the_operand_buffer():
    s = gr.make_spec(14, 9, 9, tb=1, kmode=2, c_in_a_col=0)
    size = gr.buffer_sizes(s)[0]
    req, forb, eith = gr.masks(s, size, 4)
    assert req.sum() == 14 * 9 and not eith.any() and forb.sum() == size - 14 * 9
    assert req[s["a_off"]] and req[s["a_off"] + 13 * s["lda"] + 8] and not req[s["a_off"] + 9]


def test_check_sees_wrong_values_stray_writes_and_nan():
    s = gr.make_spec(9, 9, 5, lower_only=1, alpha=0.5, beta=-2.0)
    A, B, C0 = gr.make_operands(s, np.random.default_rng(3), blk=4)
    exp = gr.expected(s, A, B, C0, blk=4)
    idx = gr.c_index(s)
    good = C0.copy()
    good[idx] = np.where(np.arange(9)[None, :] // 2 <= np.arange(9)[:, None] // 2, exp, C0[idx])     # a 2-wide tiling
    gr.check(s, good, C0, exp, blk=4)
    full = C0.copy()
    tiles = np.arange(9)[None, :] // 4 <= np.arange(9)[:, None] // 4
    full[idx] = np.where(tiles, exp, C0[idx])
    gr.check(s, full, C0, exp, blk=4)
    # (values are multiples of 1/2 here: + 0.25 is neither the exact value nor any initial one)
    for where, value in [(idx[0, 5, 2], exp[0, 5, 2] + 0.25), (idx[0, 1, 6], 0.25), (idx[0, 0, 8] + 1, 1.0), (0, 0.0),
                         (idx[0, 1, 2], exp[0, 1, 2] + 0.25), (idx[0, 1, 2], np.nan), (idx[0, 4, 4], np.nan)]:
        bad = full.copy()
        bad[where] = value
        with pytest.raises(AssertionError):
            gr.check(s, bad, C0, exp, blk=4)


def test_gpu_cases_stay_exact():
    """Exactness holds while no intermediate, in units of its granularity, reaches 2^53 -- for every case of the GPU test's
    tables, at the CU counts of one MI355X and of four times that."""
    worst = 0.0
    for n_cu in (256, 1024):
        for s in gr.all_exact_cases(n_cu):
            assert s["K"] <= 1300
            worst = max(worst, gr.exactness_bound(s))
    assert worst < 2.0 ** 53
    # and the largest case's expectation itself, computed, is a set of small integers-over-two
    s = max(gr.kmode_cases(), key=lambda c: c["K"])
    A, B, C0 = gr.make_operands(s, np.random.default_rng(0))
    exp = gr.expected(s, A, B, C0)
    assert np.abs(exp).max() < 2.0 ** 53 and np.array_equal(exp * 2, np.round(exp * 2))
    assert np.abs(exp).max() <= gr.exactness_bound(s)
