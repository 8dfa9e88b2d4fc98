"""What one launch of the fp64 GEMM (csrc/dgemm.hip, through mln_diag_dgemm_run) has to leave in memory, in plain NumPy.

The operands are small integers stored as doubles (uniform in [-4, 4], K <= 1300) and alpha, beta, beta / alpha are powers
of two: every product, every partial sum in ANY order and the scaled result are exactly representable, so the right C is one
bit pattern, `alpha * (op(A) @ op(B)) + beta * C0` in NumPy produces it, and every tiling, k-split, batch count and kernel
choice has to reproduce it -- there is no tolerance.  Everything the GEMM's contract says is never used is NaN ("poison"): a
kernel that reads it into a stored element, or writes where it must not, is seen.  Test infrastructure only: the product
never imports it.

A spec is a dict with the fields of mln_gemm_spec (see `make_spec`).  op(A) is M x K, op(B) is K x N:
  ta = 0: A stored M x K;  ta = 1: stored K x M.   tb = 0: B stored K x N;  tb = 1: stored N x K.
K-range modes, on blocks of `blk` = 128 rows / columns (smaller in the host test, so that 20 x 20 reaches every rule):
  1: op(A) block-diagonal (K = M)    2: op(B) block-diagonal (K = N)    3: op(A) lower triangular (K = M)
  4: op(B) upper triangular (K = N)  7: both lower triangular, lower tiles of the product (M = N = K)
"""
import numpy as np

BLK = 128
VMAX = 4          # operands are integers in [-VMAX, VMAX]
DEFAULTS = dict(ta=0, tb=0, lower_only=0, kmode=0, split_k=1, batch=1, mix=1, sum_partials=0, a_off=0, b_off=0, c_off=0,
                bsa=0, bsb=0, bsc=0, c_in_a_col=-1, c_in_b_off=-1, alpha=1.0, beta=0.0)


def stored_shapes(s):
    """((rows, cols) of A as stored, (rows, cols) of B as stored)"""
    return ((s["K"], s["M"]) if s["ta"] else (s["M"], s["K"])), ((s["N"], s["K"]) if s["tb"] else (s["K"], s["N"]))


def make_spec(M, N, K, align="even", **kw):
    """A complete spec.  Leading dimensions and offsets left out are chosen so that there IS padding and a lead-in to poison:
    align = "even": even leading dimensions and offsets (16-byte loads possible); "odd_ld": odd lda / ldb; "odd_off": odd
    a_off / b_off (a base that is 8- but not 16-byte aligned).  ldc is odd and c_off = 5 unless given."""
    s = dict(DEFAULTS, M=M, N=N, K=K)
    s.update(kw)
    (ra, ca), (rb, cb) = stored_shapes(s)
    even = lambda v: v + 2 + (v % 2)
    s.setdefault("lda", even(ca) + (align == "odd_ld"))
    s.setdefault("ldb", even(cb) + 2 + (align == "odd_ld"))
    if "a_off" not in kw:
        s["a_off"] = 3 if align == "odd_off" else 2
    if "b_off" not in kw:
        s["b_off"] = 5 if align == "odd_off" else 4
    in_place = s["c_in_a_col"] >= 0 or s["c_in_b_off"] >= 0
    if in_place:
        s["ldc"] = s["lda"] if s["c_in_a_col"] >= 0 else s["ldb"]
        s["c_off"] = 0
    else:
        s.setdefault("ldc", N + 3)
        if "c_off" not in kw:
            s["c_off"] = 5
    if s["batch"] > 1:
        if not s["bsa"]:
            s["bsa"] = ra * s["lda"] + 6
        if not s["bsb"]:
            s["bsb"] = rb * s["ldb"] + 4
        if not s["bsc"]:
            s["bsc"] = s["split_k"] * M * s["ldc"] + 7
    return s


def buffer_sizes(s):
    (ra, _), (rb, _) = stored_shapes(s)
    nb = s["batch"]
    return (s["a_off"] + (nb - 1) * s["bsa"] + ra * s["lda"], s["b_off"] + (nb - 1) * s["bsb"] + rb * s["ldb"],
            s["c_off"] + (nb - 1) * s["bsc"] + s["split_k"] * s["M"] * s["ldc"])


def used(s, blk=BLK):
    """(uA M x K, uB K x N, zA, zB): u* = the elements of op(A) / op(B) that lie inside the K range of SOME tile (everything
    else may be poison); z* = the elements inside which must be true zeros, so that tiles of blk and of blk / 2 mean the same
    product."""
    M, N, K, km = s["M"], s["N"], s["K"], s["kmode"]
    r, ka = np.arange(M)[:, None], np.arange(K)[None, :]
    kb, c = np.arange(K)[:, None], np.arange(N)[None, :]
    uA, uB = np.ones((M, K), bool), np.ones((K, N), bool)
    zA, zB = np.zeros((M, K), bool), np.zeros((K, N), bool)
    if km == 1:
        uA = ka // blk == r // blk
    elif km == 2:
        uB = kb // blk == c // blk
    if km in (3, 7):
        uA = ka < (r // blk + 1) * blk
        zA = uA & (ka > r)
    if km == 4:
        uB = kb < (c // blk + 1) * blk
        zB = uB & (kb > c)
    if km == 7:
        uB = kb >= (c // blk) * blk
        zB = uB & (kb < c)
    return uA, uB, zA, zB


def logical_operands(s, rng, blk=BLK, integers=True):
    """(opA [batch, M, K], opB [batch, K, N], C [batch, M, N]) with the structure the K-range mode asks for.  Elements outside
    `used` hold ordinary values here: `embed` turns them into poison, `expected` ignores them."""
    nb, M, N, K = s["batch"], s["M"], s["N"], s["K"]
    if integers:
        draw = lambda *shape: rng.integers(-VMAX, VMAX + 1, size=shape).astype(np.float64)
    else:   # full-mantissa normal numbers
        draw = lambda *shape: rng.standard_normal(shape)
    opA, opB, Cl = draw(nb, M, K), draw(nb, K, N), draw(nb, M, N)
    _, _, zA, zB = used(s, blk)
    opA[:, zA] = 0.0
    opB[:, zB] = 0.0
    return opA, opB, Cl


def c_index(s, part=0):
    """flat indices [batch, M, N] of C's elements in the buffer that holds C (the A / B buffer when in place)"""
    if s["c_in_a_col"] >= 0:
        base, ld = s["a_off"] + s["c_in_a_col"], s["lda"]
    elif s["c_in_b_off"] >= 0:
        base, ld = s["b_off"] + s["c_in_b_off"], s["ldb"]
    else:
        base, ld = s["c_off"], s["ldc"]
    b, r, c = np.arange(s["batch"])[:, None, None], np.arange(s["M"])[None, :, None], np.arange(s["N"])[None, None, :]
    return base + part * s["M"] * ld + b * s["bsc"] + r * ld + c


def embed(s, opA, opB, Cl, poison=True, blk=BLK):
    """flat buffers (A, B, C0): the logical operands in their stored layout inside NaN.  C0 is None in place."""
    na, nbuf, nc = buffer_sizes(s)
    (ra, ca), (rb, cb) = stored_shapes(s)
    uA, uB, _, _ = used(s, blk)
    A, B = np.full(na, np.nan), np.full(nbuf, np.nan)
    for b in range(s["batch"]):
        a = np.where(uA, opA[b], np.nan) if poison else opA[b]
        bb = np.where(uB, opB[b], np.nan) if poison else opB[b]
        a, bb = (a.T if s["ta"] else a), (bb.T if s["tb"] else bb)
        o = s["a_off"] + b * s["bsa"]
        A[o:o + ra * s["lda"]].reshape(ra, s["lda"])[:, :ca] = a
        o = s["b_off"] + b * s["bsb"]
        B[o:o + rb * s["ldb"]].reshape(rb, s["ldb"])[:, :cb] = bb
    if s["c_in_a_col"] >= 0 or s["c_in_b_off"] >= 0:
        return A, B, None
    C0 = np.full(nc, np.nan)
    if s["beta"] != 0.0 and s["split_k"] <= 1:
        C0[c_index(s)] = Cl
    return A, B, C0


def make_operands(s, rng, poison=True, blk=BLK):
    return embed(s, *logical_operands(s, rng, blk), poison=poison, blk=blk)


def extract(s, A, B, blk=BLK):
    """(opA, opB) [batch, M, K] / [batch, K, N] read back from the buffers, with zeros where no tile looks"""
    (ra, ca), (rb, cb) = stored_shapes(s)
    uA, uB, _, _ = used(s, blk)
    opA, opB = [], []
    for b in range(s["batch"]):
        o = s["a_off"] + b * s["bsa"]
        a = A[o:o + ra * s["lda"]].reshape(ra, s["lda"])[:, :ca]
        o = s["b_off"] + b * s["bsb"]
        bb = B[o:o + rb * s["ldb"]].reshape(rb, s["ldb"])[:, :cb]
        opA.append(np.where(uA, a.T if s["ta"] else a, 0.0))
        opB.append(np.where(uB, bb.T if s["tb"] else bb, 0.0))
    return np.stack(opA), np.stack(opB)


def expected(s, A, B, C0, blk=BLK, dtype=np.float64):
    """the exact C [batch, M, N]: alpha * op(A) op(B) + beta * C0, beta ignored for split_k > 1 (the partials sum to it; the
    caller adds beta * out).  A, B, C0: the buffers as they were BEFORE the launch (in place: C0 is the buffer C lies in)."""
    opA, opB = extract(s, A, B, blk)
    assert not (np.isnan(opA).any() or np.isnan(opB).any())
    prod = np.matmul(opA.astype(dtype), opB.astype(dtype))
    out = dtype(s["alpha"]) * prod
    if s["beta"] != 0.0 and s["split_k"] <= 1:
        out = out + dtype(s["beta"]) * C0[c_index(s)].astype(dtype)
    return out


def masks(s, size, blk=BLK):
    """(required, forbidden, either) over the `size` elements of the buffer that holds C.
    required: must hold the exact value.  forbidden: must keep the bits they had.  either: the rest of the diagonal blocks
    of a triangle of tiles, which a blk-wide tiling writes and a blk / 2-wide one skips: exact value or untouched."""
    r, c = np.arange(s["M"])[:, None], np.arange(s["N"])[None, :]
    lo = s["lower_only"]
    if lo == 0:
        req, forb = np.ones((s["M"], s["N"]), bool), np.zeros((s["M"], s["N"]), bool)
    elif lo == 1:
        req, forb = c <= r, c // blk > r // blk
    elif lo == 2:
        req, forb = c // blk < r // blk, c // blk > r // blk
    else:
        req, forb = c >= r, c // blk < r // blk
    required, either = np.zeros(size, bool), np.zeros(size, bool)
    for p in range(s["split_k"]):
        idx = c_index(s, p)
        required[idx] = req[None]
        either[idx] = (~req & ~forb)[None]
    return required, ~(required | either), either


def check(s, got, init, exp, blk=BLK):
    """The four assertions of every exact case.  got / init: the buffer that holds C after / before the launch."""
    required, forbidden, either = masks(s, got.size, blk)
    idx = c_index(s)
    bits = lambda a: a.view(np.uint64)
    g = got[idx]
    bad = required[idx] & ~(g == exp)
    assert not bad.any(), f"{int(bad.sum())} wrong values, first at (batch, row, col) = {tuple(map(int, np.argwhere(bad)[0]))}: " \
                          f"{float(g[bad][0])!r} instead of {float(exp[bad][0])!r}"
    touched = forbidden & (bits(got) != bits(init))
    assert not touched.any(), f"{int(touched.sum())} elements written outside the contract, first at buffer index " \
                              f"{int(np.flatnonzero(touched)[0])} (C starts at {int(idx.flat[0])}, ld {int(idx[0, 1, 0] - idx[0, 0, 0]) if s['M'] > 1 else 0})"
    e = either[idx] & ~((g == exp) | (bits(g) == bits(init[idx])))
    assert not e.any(), f"{int(e.sum())} diagonal-block elements neither exact nor untouched, first at {tuple(map(int, np.argwhere(e)[0]))}"
    fresh_nan = np.isnan(got) & ~np.isnan(init)
    assert not fresh_nan.any(), f"NaN appeared at buffer index {int(np.flatnonzero(fresh_nan)[0])}"


def exactness_bound(s):
    """largest |value| / granularity any intermediate of any summation order can reach: it must stay below 2^53 for "exact"
    to hold.  The accumulator holds (beta / alpha) * C0 plus up to K products of two integers <= VMAX, the result alpha times
    that (or beta * C0 when alpha is zero); alpha, beta and beta / alpha must be powers of two (or zero), so every value is
    a multiple of the granularity: the smallest of the factors below one."""
    a, b = abs(s["alpha"]), abs(s["beta"])
    bs = b / a if a else 0.0
    for v in (a, b, bs):
        assert v == 0.0 or np.frexp(v)[0] == 0.5, f"{v} is not a power of two"
    acc_mag, acc_gran = s["K"] * VMAX * VMAX + bs * VMAX, min(1.0, bs or 1.0)
    out_mag, out_gran = max(a * acc_mag, b * VMAX), min(a * acc_gran or 1.0, b or 1.0, 1.0)
    return max(acc_mag / acc_gran, out_mag / out_gran)


def kernel_spec(s):
    """the fields mln_diag_dgemm_run takes"""
    names = list(DEFAULTS) + ["M", "N", "K", "lda", "ldb", "ldc"]
    return {k: s[k] for k in names}


# ---- the case tables of tests/test_gpu_gemm_reference.py (here, so that the host test can check the exactness condition) ----
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
ALIGNS = ["even", "odd_ld", "odd_off"]
# (1, 1, 1) .. one element; (64, 64, 8): one quadrant and a partial k-tile; 192 / 256 / 384: K ranges that are a multiple of 64
# and at least 128 (the four-deep ring of the quadrant kernel); the rest: edges in every dimension, more than one tile
EDGE_SHAPES = [(1, 1, 1), (1, 300, 5), (17, 1, 33), (64, 64, 8), (65, 63, 17), (129, 127, 31), (130, 70, 40), (257, 259, 130),
               (300, 200, 192), (200, 136, 256), (384, 384, 384)]
SCALINGS = [(1.0, 0.0), (0.5, -2.0), (-1.0, 1.0), (0.0, 2.0), (2.0, 0.0)]


def layout_cases():
    return [make_spec(M, N, K, align=al, ta=ta, tb=tb) for (M, N, K) in EDGE_SHAPES for (ta, tb) in LAYOUTS for al in ALIGNS]


def scaling_cases():
    return [make_spec(M, N, K, ta=ta, tb=0, alpha=a, beta=b)
            for (M, N, K) in [(130, 70, 40), (257, 259, 130)] for ta in (0, 1) for (a, b) in SCALINGS]


def triangle_cases():
    # NT like the Cholesky trailing update (linalg.hip: A22 -= P P^T on lower tiles); non-square tile grids last
    shapes = [(129, 129), (300, 300), (645, 645), (400, 200), (200, 400)]
    return [make_spec(M, N, 40, ta=0, tb=1, lower_only=lo, alpha=a, beta=b)
            for (M, N) in shapes for lo in (1, 2, 3) for (a, b) in [(-1.0, 1.0), (2.0, 0.0)]]


def kmode_cases():
    out = []
    for m in (300, 768):      # block-diagonal operand: the triangular-inverse build (lower_only 2) and the final launches of
        for lo in (0, 1, 2, 3):    # the block solves (lower_only 0 / 1 / 3) in linalg.hip are NN, NT and TN; TT for completeness
            n = m if lo else 260
            for (ta, tb) in LAYOUTS:
                out.append(make_spec(m, n, m, ta=ta, tb=tb, kmode=1, lower_only=lo, alpha=-1.0))
                out.append(make_spec(n, m, m, ta=ta, tb=tb, kmode=2, lower_only=lo, alpha=-1.0))
    for m in (300, 900):
        for (ta, tb) in LAYOUTS:
            out.append(make_spec(m, 200, m, ta=ta, tb=tb, kmode=3, alpha=0.5, beta=-2.0))
            out.append(make_spec(200, m, m, ta=ta, tb=tb, kmode=4, alpha=0.5, beta=-2.0))
    for m in (300, 900, 1280):      # (the large ones: both operands as stored, both transposed)
        for (ta, tb) in (LAYOUTS if m == 300 else [(0, 0), (1, 1)]):
            out.append(make_spec(m, m, m, ta=ta, tb=tb, kmode=7, lower_only=1, alpha=0.5, beta=-2.0))
    return out


def split_cases():
    # (130, 70, 40) in 7: chunks of 16, four of them empty; the last: the Gram of the preconditioner (TN, lower tiles)
    return [make_spec(130, 70, 40, split_k=7, alpha=0.5), make_spec(300, 300, 1000, tb=1, split_k=3, alpha=-1.0),
            make_spec(257, 257, 700, ta=1, lower_only=1, split_k=5, alpha=2.0)]


def mixed_cases(n_cu):
    """launches in which the mixed kernel serves 128-tiles AND quadrants: a round is 2 n_cu / (split * batch) = 32 tiles, 36
    tiles are active"""
    out = []
    for batch in (1, 2):
        split = max(1, n_cu // 16)
        K = 16 * split + 24
        split //= batch
        if split < 1:
            continue
        out.append(make_spec(768, 768, K, tb=1, split_k=split, batch=batch, alpha=0.5, ldc=770, c_off=2))
        out.append(make_spec(1024, 1024, K, tb=1, split_k=split, batch=batch, lower_only=1, alpha=0.5, ldc=1026, c_off=2))
        if batch == 1:      # the same launch with scalar loads (odd leading dimensions)
            out.append(make_spec(768, 768, K, align="odd_ld", tb=1, split_k=split, alpha=0.5, ldc=770, c_off=2))
    return out


def batch_cases():
    return [make_spec(M, N, K, ta=ta, batch=nb, alpha=0.5, beta=-2.0)
            for (M, N, K) in [(130, 70, 40), (300, 257, 64)] for nb in (2, 3) for ta in (0, 1)]


def inplace_cases():
    out = []
    for al in ("even", "odd_ld"):
        for M in (130, 700):          # X <- X blockdiag(W)^T with one column tile (triinv_solve_right_T)
            for n in (100, 128):
                out.append(make_spec(M, n, n, align=al, tb=1, kmode=2, c_in_a_col=0))
        # one row tile: B[j0 : j0 + nb] <- W_j B[: j0 + nb] (the left-looking triinv_solve_left)
        s = make_spec(100, 300, 228, align=al)
        out.append(make_spec(100, 300, 228, align=al, c_in_b_off=128 * s["ldb"]))
        # B <- blockdiag(Dinv) B, a tile reads exactly the tile it overwrites (the right-looking triinv_solve_left)
        out.append(make_spec(300, 260, 300, align=al, kmode=1, c_in_b_off=0))
    return out


def all_exact_cases(n_cu):
    return (layout_cases() + scaling_cases() + triangle_cases() + kmode_cases() + split_cases() + mixed_cases(n_cu) +
            batch_cases() + inplace_cases())
