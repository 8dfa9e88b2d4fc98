"""The fp64 GEMM (csrc/dgemm.hip) against an exact reference in every launch mode (-m gpu).

Integer-valued operands and power-of-two scalings make the right result one bit pattern (tests/gemm_reference.py), so every
case asserts, with no tolerance: the required elements hold the exact product; everything outside M x N, outside the
requested triangle of tiles, in paddings, lead-ins and batch gaps keeps its bits; the rest of a triangle's diagonal blocks is
exact or untouched; no NaN appears where none was put -- and every operand element the contract calls unused IS NaN.  One
upload, one launch, one download per case (mln_diag_dgemm_run).  `mix` 0 runs the single-size tile kernels, 1 the launch
policy's own choice (the pipelined mixed-tile kernel wherever it serves the launch)."""
import math
import zlib

import numpy as np
import pytest

import gemm_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def _id(s):
    t = f"{'T' if s['ta'] else 'N'}{'T' if s['tb'] else 'N'}-{s['M']}x{s['N']}x{s['K']}-lda{s['lda']}-ao{s['a_off']}"
    for k, short in [("lower_only", "lo"), ("kmode", "km"), ("split_k", "sk"), ("batch", "b")]:
        if s[k] > (1 if k in ("split_k", "batch") else 0):
            t += f"-{short}{s[k]}"
    if s["c_in_a_col"] >= 0 or s["c_in_b_off"] >= 0:
        t += "-inA" if s["c_in_a_col"] >= 0 else f"-inB{s['c_in_b_off']}"
    return t + f"-a{s['alpha']:g}-b{s['beta']:g}"


_cache = {}


def _problem(s):
    """(A, B, C0, expected) of a spec, made once and shared by its `mix` variants; never modified"""
    key = tuple(sorted((k, v) for k, v in s.items() if k not in ("mix", "sum_partials")))
    if key not in _cache:
        _cache.clear()      # (the variants of one spec run back to back: one entry is enough, and the large cases do not pile up)
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        A, B, C0 = gr.make_operands(s, rng)
        held = A if s["c_in_a_col"] >= 0 else (B if s["c_in_b_off"] >= 0 else C0)
        for a in (A, B, held):
            a.setflags(write=False)
        _cache[key] = (A, B, held, gr.expected(s, A, B, held))
    return _cache[key]


def _run_exact(ctx, s, mix):
    s = dict(s, mix=mix)
    A, B, held, exp = _problem(s)
    got = ctx.diag_dgemm_run(gr.kernel_spec(s), A, B, held)
    gr.check(s, got, held, exp)


def _param(cases):
    return pytest.mark.parametrize("s", cases, ids=[_id(c) for c in cases])


MIX = pytest.mark.parametrize("mix", [0, 1])


@MIX
@_param(gr.layout_cases())
def test_layouts_and_edges(ctx, s, mix):
    """All four operand layouts, 16-byte and scalar loads (odd leading dimension; odd offset), every edge of the tiling."""
    _run_exact(ctx, s, mix)


@MIX
@_param(gr.scaling_cases())
def test_scaling(ctx, s, mix):
    """beta folded into the accumulators as beta / alpha, beta == 0 on a C that is all NaN, and alpha == 0: the only route to
    the epilogue's own beta * C."""
    _run_exact(ctx, s, mix)


@MIX
@_param(gr.triangle_cases())
def test_triangles_of_tiles(ctx, s, mix):
    """lower_only 1, 2, 3: square tile grids (the mixed kernel's enumeration) and non-square ones (it declines: fallback)."""
    _run_exact(ctx, s, mix)


@MIX
@_param(gr.kmode_cases())
def test_k_range_modes(ctx, s, mix):
    """Block-diagonal and triangular K ranges: what lies outside a tile's range is NaN in the operands."""
    _run_exact(ctx, s, mix)


@MIX
@_param(gr.batch_cases())
def test_batch(ctx, s, mix):
    """batch = 2, 3 with a NaN gap between the outputs that has to stay."""
    _run_exact(ctx, s, mix)


@MIX
@_param(gr.inplace_cases())
def test_in_place(ctx, s, mix):
    """C inside an operand (the panels of the block solves): the expectation comes from the operand as it was before."""
    _run_exact(ctx, s, mix)


def _check_partials(s, parts, C0, exp):
    required, forbidden, _ = gr.masks(s, parts.size)
    bits = lambda a: a.view(np.uint64)
    assert not (forbidden & (bits(parts) != bits(C0))).any(), "written outside the contract"
    req = required[gr.c_index(s)]
    total = np.zeros_like(exp)
    for p in range(s["split_k"]):         # fixed order, like k_sum_partials
        part = parts[gr.c_index(s, p)]
        assert np.isfinite(part[req]).all(), f"partial {p} has unwritten elements"      # an empty chunk writes zeros
        either = ~req & ~forbidden[gr.c_index(s, p)]
        assert (np.isfinite(part[either]) | (bits(part) == bits(C0[gr.c_index(s, p)]))[either]).all()
        total += np.where(req, part, 0.0)
    bad = req & (total != exp)
    assert not bad.any(), f"{int(bad.sum())} wrong sums, first at (batch, row, col) = {tuple(map(int, np.argwhere(bad)[0]))}"
    return req


def _run_split(ctx, s, mix):
    s = dict(s, mix=mix)
    A, B, C0, exp = _problem(s)
    parts = ctx.diag_dgemm_run(gr.kernel_spec(s), A, B, C0)
    _check_partials(s, parts, C0, exp)


@MIX
@_param(gr.split_cases())
def test_split_k_partials(ctx, s, mix):
    """Every k-chunk writes its partial -- zeros when the chunk is empty -- and their sum is the exact product."""
    _run_split(ctx, s, mix)


@MIX
@pytest.mark.parametrize("beta", [0.0, -2.0])
@_param(gr.split_cases())
def test_split_k_summed(ctx, s, beta, mix):
    """launch_sum_partials: out = beta * out + the partials in fixed order (beta = 0: out unread)."""
    s = dict(s, mix=mix, beta=beta, sum_partials=1)
    A, B, C0, exp = _problem(s)
    rng = np.random.default_rng(5)
    n_out = s["M"] * s["ldc"]
    out0 = np.full(n_out, np.nan) if beta == 0.0 else rng.integers(-4, 5, size=n_out).astype(np.float64)
    parts, out = ctx.diag_dgemm_run(gr.kernel_spec(s), A, B, C0, out0)
    req = _check_partials(s, parts, C0, exp)[0]
    out, out0 = (a.reshape(s["M"], s["ldc"])[:, :s["N"]] for a in (out, out0))
    want = exp[0] + (beta * out0 if beta != 0.0 else 0.0)
    assert np.array_equal(out[req], want[req])


@pytest.mark.parametrize("which,batch", [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2)],
                         ids=["768-full", "1024-lower", "768-full-scalar-loads", "768-full-batch2", "1024-lower-batch2"])
def test_mixed_launch_with_both_tile_sizes(ctx, which, batch):
    """36 active tiles where a round of 128-tiles is 32: the first 32 run as 128-tiles, four as quadrants, in ONE launch."""
    n_cu = ctx.device_info()["n_cu"]
    cases = [c for c in gr.mixed_cases(n_cu) if c["batch"] == batch]
    if not cases:
        pytest.fail(f"no mixed case for {n_cu} CUs")
    s = cases[which]
    assert 2 * n_cu // (s["split_k"] * batch) == 32, "the case is written for a CU count that is a multiple of 32"
    _run_split(ctx, s, 1)


# ---- one case whose result is NOT exact: full-mantissa operands against extended precision --------------------------------
_ROUNDING = dict(M=257, N=259, K=517, alpha=0.75, beta=-1.3)
_rounding_ref = {}


def _rounding_problem():
    if not _rounding_ref:
        s = gr.make_spec(_ROUNDING["M"], _ROUNDING["N"], _ROUNDING["K"], alpha=0.75, beta=-1.3)
        opA, opB, Cl = gr.logical_operands(s, np.random.default_rng(11), integers=False)
        a, b = abs(s["alpha"]), abs(s["beta"])
        # recursive summation of K products ((K - 1 additions + K multiplications: gamma_K), plus the roundings of
        # beta / alpha, its product with C, the addition of that to the sum and the final scaling
        bound = (s["K"] + 6) * 2.0 ** -53 * (a * (np.abs(opA[0]) @ np.abs(opB[0])) + b * np.abs(Cl[0]))
        if np.finfo(np.longdouble).nmant >= 63:
            L = np.longdouble
            ref = L(s["alpha"]) * (opA[0].astype(L) @ opB[0].astype(L)) + L(s["beta"]) * Cl[0].astype(L)
            corner = (s["M"], s["N"])
        else:       # no extended precision on this host: exactly rounded sums of the exact products' halves, on a corner
            corner = (40, 40)
            ref = np.empty(corner)
            for i in range(40):
                for j in range(40):
                    terms = [s["alpha"] * x * y for x, y in zip(opA[0, i], opB[0, :, j])]      # (one rounding each: in the bound)
                    ref[i, j] = math.fsum(terms + [s["beta"] * Cl[0, i, j]])
        _rounding_ref.update(ops=(opA, opB, Cl), ref=ref, bound=bound, corner=corner)
    return _rounding_ref


@MIX
@pytest.mark.parametrize("ta,tb", gr.LAYOUTS)
def test_rounding_error_within_the_summation_bound(ctx, ta, tb, mix):
    """|C - reference| <= (K + 6) 2^-53 (|alpha| |A| |B| + |beta| |C0|) per element, the reference in np.longdouble."""
    p = _rounding_problem()
    s = gr.make_spec(_ROUNDING["M"], _ROUNDING["N"], _ROUNDING["K"], ta=ta, tb=tb, alpha=0.75, beta=-1.3, mix=mix)
    A, B, C0 = gr.embed(s, *p["ops"])
    got = ctx.diag_dgemm_run(gr.kernel_spec(s), A, B, C0)
    required, forbidden, _ = gr.masks(s, got.size)
    assert np.array_equal(got.view(np.uint64)[forbidden], C0.view(np.uint64)[forbidden])
    m, n = p["corner"]
    g = got[gr.c_index(s)][0][:m, :n]
    assert np.isfinite(got[gr.c_index(s)]).all()
    err = np.abs((g.astype(np.longdouble) - p["ref"][:m, :n]).astype(np.float64))
    worst = (err / p["bound"][:m, :n]).max()
    print(f"largest error / bound = {worst:.3g}")
    assert worst <= 1.0, worst


def test_malformed_specs_are_refused(ctx):
    """A spec whose accesses do not fit the buffers is an error code, never a launch."""
    from mellon_amd._lib import MellonHipError
    s = gr.make_spec(65, 63, 17, beta=1.0)
    A, B, C0, _ = _problem(s)
    for change in [dict(M=66), dict(N=s["ldc"] + 1), dict(K=18), dict(lda=s["lda"] + 1), dict(ldb=s["ldb"] + 1), dict(ldc=s["ldc"] + 1),
                   dict(a_off=s["a_off"] + 1), dict(b_off=s["b_off"] + 1), dict(c_off=s["c_off"] + 1), dict(split_k=2),
                   dict(batch=2, bsa=0, bsb=0, bsc=0), dict(kmode=5), dict(lower_only=4), dict(ta=1, M=500), dict(tb=1, N=500),
                   dict(c_in_a_col=0, ldc=s["lda"]), dict(c_in_b_off=s["ldb"] - 3, ldc=s["ldb"]), dict(sum_partials=1), dict(a_off=-1)]:
        with pytest.raises(MellonHipError):
            ctx.diag_dgemm_run(dict(gr.kernel_spec(s), **change), A, B, C0)
