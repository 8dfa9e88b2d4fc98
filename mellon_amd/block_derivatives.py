"""Analytic derivatives of block-evaluated covariance trees (base_cov.BlockCov): `Covariance.k_grad`, the gradient and
the Hessian of the predictive mean for trees that are not one device program -- more than MAX_LEAVES leaves, a stack
deeper than MAX_DEPTH, or user-defined leaves (reference base_cov.py:317-497 carries k_grad through Add / Mul / Pow,
base_predictor.py:490-539 differentiates `_mean`).

For one pair (x_i, c_j) the covariance is P(k_1 .. k_L) over its leaves.  With a_l = dP/dk_l and b_ll' = d2P/dk_l dk_l'

    grad_i = sum_j w_j sum_l a_l grad k_l
    H_i    = sum_j w_j [ sum_l a_l hess k_l + sum_{l,l'} b_ll' grad k_l grad k_l'^T ]

which is what csrc/cov_kernels.hip evaluates for one program, its a / b held in registers.  Here they are (rows x ld)
blocks: per row block of queries the tree is walked bottom-up, every node carrying its value block and its first (and,
for the Hessian, second) derivatives with respect to the leaves beneath it

    Add        union of the children's derivative sets
    Mul(u, v)  v du, u dv ;  v d2u, u d2v and the cross products du/dl dv/dl'
    Pow(u, p)  p u^(p-1) du ;  p (p-1) u^(p-2) du du + p u^(p-1) d2u

A leaf's derivative with respect to itself is the number 1.0, never a block; the same leaf object appearing twice counts
as two leaves; `active_dims` compose exactly as in Covariance._emit / _block.  The block arithmetic goes through a small
backend (`mul`, `add`, `pow`, `scale`): `DeviceBlocks` is mln_ewise on DeviceArrays, `NumpyBlocks` the same on host arrays
(the walk is testable without a GPU).  The leaf factors and the final contractions are csrc/cov_block_deriv.hip.
"""
import ctypes as C

import numpy as np

from . import _lib
from .util import compose_active_dims

BLOCK_BYTES = 1 << 31        # live blocks of one row block stay within 2 GiB, like launch_predict_hessian's coefficients


# ---- the tree as data ------------------------------------------------------------------------------------------
class LeafRecord:
    """One leaf occurrence: `cols` are the original columns visible at the node (what a user-defined k / k_grad sees),
    `dims` the columns a built-in leaf is evaluated on (its own active_dims applied), as `_emit` would give them."""

    def __init__(self, node, cols):
        self.node, self.cols = node, np.asarray(cols)
        self.user = node._user_defined()
        self.dims = None if self.user else np.ascontiguousarray(compose_active_dims(cols, node.active_dims), dtype=np.int32)
        self.kind = None if self.user else int(node._kind)
        self.ls = float(getattr(node, "ls", 1.0))
        self.alpha = float(getattr(node, "alpha", 1.0))

    @property
    def linear(self):
        return self.kind == _lib.K_LINEAR

    def has_k_grad(self):
        from .base_cov import Covariance
        return type(self.node).k_grad is not Covariance.k_grad


def collect_leaves(cov, d):
    """(leaves, plan): the leaf occurrences of the tree in postfix order and the tree over them --
    ("leaf", index) | (op, left_plan, right_plan) | (op, left_plan, ("const", value))."""
    from .base_cov import CovariancePair
    leaves = []

    def visit(node, cols):
        if isinstance(node, CovariancePair):
            cols = compose_active_dims(cols, node.active_dims)
            left = visit(node.left, cols)
            if callable(node.right):
                if node._op == _lib.OP_POW:
                    raise NotImplementedError("covariance ** covariance is not defined")
                right = visit(node.right, cols)
            else:
                right = ("const", float(node.right))
            return (node._op, left, right)
        leaves.append(LeafRecord(node, cols))
        return ("leaf", len(leaves) - 1)

    plan = visit(cov, np.arange(d))
    return leaves, plan


# ---- block arithmetic ------------------------------------------------------------------------------------------
class NumpyBlocks:
    """Host backend of the walk."""

    def mul(self, a, b):
        return a * b

    def add(self, a, b):
        return a + b

    def pow(self, a, p):
        return a ** p

    def scale(self, a, s):
        return a * s


class _Block:
    """A DeviceArray on loan from DeviceBlocks' pool: it goes back when the last reference to the block dies."""
    __slots__ = ("arr", "pool")

    def __init__(self, arr, pool):
        self.arr, self.pool = arr, pool

    @property
    def ptr(self):
        return self.arr.ptr

    def __del__(self):
        self.pool.append(self.arr)


class DeviceBlocks:
    """mln_ewise on (rows x ld) DeviceArrays; every operation writes a fresh block (operands are never modified, so a
    derivative may be shared between nodes).  Blocks of finished row blocks are reused."""

    def __init__(self, ctx, max_rows, ld):
        self.ctx, self.max_rows, self.ld, self.rows = ctx, int(max_rows), int(ld), int(max_rows)
        self._pool = []

    def new(self):
        arr = self._pool.pop() if self._pool else self.ctx.empty((self.max_rows, self.ld))
        return _Block(arr, self._pool)

    def _ewise(self, op, a, b, scalar):
        out = self.new()
        self.ctx._check(self.ctx.lib.mln_ewise(self.ctx.handle, op, a.ptr, None if b is None else b.ptr, float(scalar),
                                               out.ptr, self.rows * self.ld))
        return out

    def mul(self, a, b):
        return self._ewise(_lib.OP_MUL, a, b, 0.0)

    def add(self, a, b):
        if isinstance(b, float):
            return self._ewise(_lib.OP_ADD, a, None, b)
        return self._ewise(_lib.OP_ADD, a, b, 0.0)

    def pow(self, a, p):
        return self._ewise(_lib.OP_POW, a, None, p)

    def scale(self, a, s):
        return self._ewise(_lib.OP_MUL, a, None, s)

    def upload(self, host, m):
        """A (rows x m) host array as a block (pad columns zero)."""
        buf = np.zeros((self.rows, self.ld))
        buf[:, :m] = host
        out = self.new()
        self.ctx._check(self.ctx.lib.mln_memcpy(self.ctx.handle, out.ptr, buf.ctypes.data, buf.nbytes))
        return out

    def download(self, blk, m):
        buf = np.empty((self.rows, self.ld))
        self.ctx._check(self.ctx.lib.mln_memcpy(self.ctx.handle, buf.ctypes.data, blk.ptr, buf.nbytes))
        return buf[:, :m]


def _num(a):
    return isinstance(a, float)


def _mul(be, a, b):
    """Product of two coefficients, each a block or a number."""
    if _num(a) and _num(b):
        return a * b
    if _num(a):
        a, b = b, a
    if _num(b):
        return a if b == 1.0 else be.scale(a, b)
    return be.mul(a, b)


def _add(be, a, b):
    if _num(a) and _num(b):
        return a + b
    if _num(a):
        a, b = b, a
    return be.add(a, b)


def _as_block(be, a, like):
    """A number as a constant block shaped like the (finite) block `like`."""
    return be.add(be.scale(like, 0.0), a) if _num(a) else a


def propagate(plan, values, be, second=False):
    """(value, first, second) of the node `plan`: first[l] = d node / d k_l, second[(l, l')] (l <= l') =
    d2 node / d k_l d k_l' (the mixed partial once), as blocks or numbers; entries that vanish identically are absent."""
    if plan[0] == "leaf":
        return values[plan[1]], {plan[1]: 1.0}, {}
    op, lplan, rplan = plan
    u, du, d2u = propagate(lplan, values, be, second)
    if rplan[0] == "const":
        s = rplan[1]
        if op == _lib.OP_ADD:
            return be.add(u, s), du, d2u
        if op == _lib.OP_MUL:
            return (be.scale(u, s), {l: _mul(be, t, s) for l, t in du.items()},
                    {k: _mul(be, t, s) for k, t in d2u.items()})
        f1 = be.scale(be.pow(u, s - 1.0), s)                              # p u^(p-1)
        first = {l: _mul(be, f1, t) for l, t in du.items()}
        sec = {}
        if second:
            f2 = be.scale(be.pow(u, s - 2.0), s * (s - 1.0))              # p (p-1) u^(p-2)
            ls = sorted(du)
            for a, l in enumerate(ls):
                for lp in ls[a:]:
                    t = _mul(be, f2, _mul(be, du[l], du[lp]))
                    if (l, lp) in d2u:
                        t = _add(be, t, _mul(be, f1, d2u[(l, lp)]))
                    sec[(l, lp)] = t
        return be.pow(u, s), first, sec
    v, dv, d2v = propagate(rplan, values, be, second)
    if op == _lib.OP_ADD:
        return be.add(u, v), {**du, **dv}, {**d2u, **d2v}
    if op != _lib.OP_MUL:
        raise NotImplementedError("covariance ** covariance is not defined")
    first = {l: _mul(be, v, t) for l, t in du.items()}
    first.update({l: _mul(be, u, t) for l, t in dv.items()})
    sec = {}
    if second:
        sec = {k: _mul(be, v, t) for k, t in d2u.items()}
        sec.update({k: _mul(be, u, t) for k, t in d2v.items()})
        for l, tu in du.items():                                          # leaves of u come before those of v: l < l'
            for lp, tv in dv.items():
                sec[(l, lp)] = _mul(be, tu, tv)
    return be.mul(u, v), first, sec


# ---- device side -----------------------------------------------------------------------------------------------
def _pad16(m):
    return ((int(m) + 15) // 16) * 16


def _rows_per_block(limit, ld, n_live, extra_per_row=0):
    """Query rows per block so that `n_live` (rows x ld) blocks (+ extra_per_row doubles per row) fit BLOCK_BYTES."""
    rows = BLOCK_BYTES // (8 * (ld * n_live + extra_per_row))
    rows = max(64, (rows // 64) * 64)
    return int(min(int(limit), rows))


class _LeafArgs:
    """The ctypes side of the built-in leaves: one mln_leaf array (accumulation entries) and a one-leaf descriptor each
    (mln_leaf_factors)."""

    def __init__(self, leaves):
        from .base_cov import LoweredCov
        self.builtin = [i for i, lf in enumerate(leaves) if not lf.user]
        recs = [leaves[i] for i in self.builtin]
        self.all = LoweredCov([(lf.kind, lf.ls, lf.alpha, lf.dims) for lf in recs], [(_lib.OP_LEAF, 0, 0.0)]) if recs else None
        self.single = {i: LoweredCov([(lf.kind, lf.ls, lf.alpha, lf.dims)], [(_lib.OP_LEAF, 0, 0.0)])
                       for i, lf in zip(self.builtin, recs)}

    def pointers(self, blocks):
        arr = (C.c_void_p * max(1, len(blocks)))()
        for i, b in enumerate(blocks):
            arr[i] = None if b is None else b.ptr
        return arr


def _leaf_factors(ctx, be, largs, i, x_dev, rows, c_dev, m, d, exact, want_h):
    K, g, h = be.new(), be.new(), (be.new() if want_h else None)
    ctx._check(ctx.lib.mln_leaf_factors(ctx.handle, largs.single[i].ref, x_dev.ptr, rows, c_dev.ptr, m, d, int(exact), be.ld,
                                        K.ptr, g.ptr, None if h is None else h.ptr))
    return K, g, h


def _user_value(be, lf, xb, c):
    xs, cs = np.ascontiguousarray(xb[:, lf.cols]), np.ascontiguousarray(c[:, lf.cols])
    vals = np.asarray(type(lf.node).k(lf.node, xs, cs), dtype=np.float64)
    if vals.shape != (xb.shape[0], c.shape[0]):
        raise ValueError(f"{type(lf.node).__name__}.k returned shape {vals.shape}, expected {(xb.shape[0], c.shape[0])}")
    return be.upload(vals, c.shape[0])


def _user_k_grad(lf, x, y):
    """The user's k_grad(x)(y): (n, m, len(cols)), derivative with respect to y on the columns visible at the leaf."""
    xs, ys = np.ascontiguousarray(x[:, lf.cols]), np.ascontiguousarray(y[:, lf.cols])
    T = np.asarray(type(lf.node).k_grad(lf.node, xs)(ys), dtype=np.float64)
    if T.shape != (x.shape[0], y.shape[0], len(lf.cols)):
        raise ValueError(f"{type(lf.node).__name__}.k_grad returned shape {T.shape}, expected "
                         f"{(x.shape[0], y.shape[0], len(lf.cols))}")
    return T


def _require_k_grad(leaves, what):
    for lf in leaves:
        if lf.user and not lf.has_k_grad():
            raise NotImplementedError(
                f"{what}: the user-defined kernel {type(lf.node).__name__} defines k() only.  Give it a "
                "k_grad(x) -> (y -> (n, m, d)) like the built-in kernels have; a Python k() is not differentiated "
                "automatically.")


def _host(a):
    return a.to_host() if isinstance(a, _lib.DeviceArray) else np.ascontiguousarray(a, dtype=np.float64)


def _values_and_factors(ctx, be, largs, leaves, xb, x_dev, c, c_dev, exact, want_h):
    m, d = c.shape
    vals, g, h = [], {}, {}
    for i, lf in enumerate(leaves):
        if lf.user:
            vals.append(_user_value(be, lf, xb, c))
        else:
            K, g[i], h[i] = _leaf_factors(ctx, be, largs, i, x_dev, xb.shape[0], c_dev, m, d, exact, want_h)
            vals.append(K)
    return vals, g, h


def predict_gradient(ctx, bc, xnew, centers, w):
    """sum_j w_j d cov(x_i, c_j) / d x_i for a BlockCov: (n, d)."""
    x, c, w = _host(xnew), _host(centers), np.ascontiguousarray(w, dtype=np.float64)
    leaves, plan = collect_leaves(bc.cov, bc.d)
    _require_k_grad(leaves, "predict_gradient")
    largs = _LeafArgs(leaves)
    (n, d), m, L = x.shape, c.shape[0], len(leaves)
    out = np.zeros((n, d))
    if n == 0 or m == 0:
        return out
    ld = _pad16(m)
    nb = _rows_per_block(bc.rows_per_block, ld, 4 * L + 6)
    be = DeviceBlocks(ctx, min(nb, n), ld)
    c_dev, w_dev = ctx.to_device(c), ctx.to_device(w)
    for i0 in range(0, n, nb):
        xb = np.ascontiguousarray(x[i0:i0 + nb])
        be.rows = rows = xb.shape[0]
        x_dev = ctx.to_device(xb)
        vals, g, _ = _values_and_factors(ctx, be, largs, leaves, xb, x_dev, c, c_dev, 1, False)
        _, first, _ = propagate(plan, vals, be)
        ob = out[i0:i0 + rows]
        if largs.builtin:
            Q = [_as_block(be, _mul(be, first[i], g[i]), vals[i]) for i in largs.builtin]
            ctx._check(ctx.lib.mln_block_grad_accumulate(ctx.handle, largs.all._leaves, len(Q), largs.pointers(Q), ld,
                                                         x_dev.ptr, rows, d, c_dev.ptr, m, w_dev.ptr, ob.ctypes.data))
            del Q
        for i, lf in enumerate(leaves):
            if not lf.user:
                continue
            # d k(x_i, c_j) / d x_i = k_grad(c)(x)[j, i, :] by the symmetry of a covariance
            T = _user_k_grad(lf, c, xb)
            r = np.empty(rows)
            for k, col in enumerate(lf.cols):
                D = be.upload(T[:, :, k].T, m)
                prod = _mul(be, D, first[i])
                ctx._check(ctx.lib.mln_gemm(ctx.handle, 0, 0, rows, 1, m, 1.0, prod.ptr, ld, w_dev.ptr, 1, 0.0,
                                            r.ctypes.data, 1))
                ob[:, col] += r
        del vals, g, first
    return out


def hessian_coefficients(be, leaves, vals, g, h, a1, a2):
    """The coefficient blocks of mln_block_hess_accumulate from the walk's a1 / a2 and the leaf factors g / h:
    Qd[l] = a_l g_l (None for Linear), Qp in the order (0,0) (0,1) .. (1,1) ..: a_l h_l + a_ll gam_l^2 on the diagonal,
    a_ll' gam_l gam_l' off it, gam = g or -1 / ls for Linear; None where the coefficient vanishes identically."""
    L = len(leaves)
    gam = [(-1.0 / lf.ls) if lf.linear else g[i] for i, lf in enumerate(leaves)]
    Qd = [None if lf.linear else _as_block(be, _mul(be, a1[i], g[i]), vals[i]) for i, lf in enumerate(leaves)]
    Qp = []
    for l in range(L):
        for lp in range(l, L):
            b = a2.get((l, lp))
            t = None
            if l == lp and not leaves[l].linear:
                t = _mul(be, a1[l], h[l])
            if b is not None:
                t2 = _mul(be, b, _mul(be, gam[l], gam[lp]))
                t = t2 if t is None else _add(be, t, t2)
            Qp.append(None if t is None else _as_block(be, t, vals[l]))
    return Qd, Qp


def predict_hessian(ctx, bc, xnew, centers, w):
    """Hessian of sum_j w_j cov(x_i, c_j) in x_i for a BlockCov of built-in leaves: (n, d, d)."""
    x, c, w = _host(xnew), _host(centers), np.ascontiguousarray(w, dtype=np.float64)
    leaves, plan = collect_leaves(bc.cov, bc.d)
    for lf in leaves:
        if lf.user:
            raise NotImplementedError(
                f"predict_hessian: the tree holds the user-defined kernel {type(lf.node).__name__}.  A user's k_grad gives "
                "first derivatives only and a Python k() is not differentiated automatically, so second derivatives exist "
                "for trees of built-in kernels only.")
    largs = _LeafArgs(leaves)
    (n, d), m, L = x.shape, c.shape[0], len(leaves)
    out = np.zeros((n, d, d))
    if n == 0 or m == 0:
        return out
    ld = _pad16(m)
    nd = max(len(lf.dims) for lf in leaves)
    nb = _rows_per_block(bc.rows_per_block, ld, 5 * L + L * (L + 1) + 8, extra_per_row=_pad16(nd * nd + 2 * nd + 1) + d * d)
    be = DeviceBlocks(ctx, min(nb, n), ld)
    c_dev, w_dev = ctx.to_device(c), ctx.to_device(w)
    for i0 in range(0, n, nb):
        xb = np.ascontiguousarray(x[i0:i0 + nb])
        be.rows = rows = xb.shape[0]
        x_dev = ctx.to_device(xb)
        vals, g, h = _values_and_factors(ctx, be, largs, leaves, xb, x_dev, c, c_dev, 1, True)
        _, a1, a2 = propagate(plan, vals, be, second=True)
        Qd, Qp = hessian_coefficients(be, leaves, vals, g, h, a1, a2)
        ob = out[i0:i0 + rows]
        ctx._check(ctx.lib.mln_block_hess_accumulate(ctx.handle, largs.all._leaves, L, largs.pointers(Qd), largs.pointers(Qp),
                                                     ld, x_dev.ptr, rows, d, c_dev.ptr, m, w_dev.ptr, ob.ctypes.data))
        del vals, g, h, a1, a2, Qd, Qp
    return out


def kernel_grad(ctx, bc, x, y):
    """d cov(x_i, y_j) / d y_j for a BlockCov: (n, m, d), util.distance_grad's dist + 1e-12 denominator."""
    x, y = _host(x), _host(y)
    leaves, plan = collect_leaves(bc.cov, bc.d)
    _require_k_grad(leaves, "kernel_grad")
    largs = _LeafArgs(leaves)
    (n, d), m, L = x.shape, y.shape[0], len(leaves)
    out = np.zeros((n, m, d))
    if n == 0 or m == 0:
        return out
    ld = _pad16(m)
    nb = _rows_per_block(bc.rows_per_block, ld, 4 * L + 6, extra_per_row=m * d)
    be = DeviceBlocks(ctx, min(nb, n), ld)
    y_dev = ctx.to_device(y)
    for i0 in range(0, n, nb):
        xb = np.ascontiguousarray(x[i0:i0 + nb])
        be.rows = rows = xb.shape[0]
        x_dev = ctx.to_device(xb)
        vals, g, _ = _values_and_factors(ctx, be, largs, leaves, xb, x_dev, y, y_dev, 0, False)
        _, first, _ = propagate(plan, vals, be)
        ob = out[i0:i0 + rows]
        if largs.builtin:
            A = [_as_block(be, _mul(be, first[i], g[i]), vals[i]) for i in largs.builtin]
            ctx._check(ctx.lib.mln_block_kernel_grad(ctx.handle, largs.all._leaves, len(A), largs.pointers(A), ld, x_dev.ptr,
                                                     rows, y_dev.ptr, m, d, ob.ctypes.data))
            del A
        for i, lf in enumerate(leaves):
            if lf.user:
                a = first[i] if _num(first[i]) else be.download(first[i], m)[:, :, None]
                ob[:, :, lf.cols] += a * _user_k_grad(lf, xb, y)
        del vals, g, first
    return out
