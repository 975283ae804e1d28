"""BBOB / noisy-BBOB objectives in extended precision, and how far a correct float64 kernel may be from them.

The reference objectives (src/problem/bbob.py: sr_func, T_osz, T_asy, pen_func, F1-F24 and the Gauss / Uniform / Cauchy noise models) are
restated once, in `_core`, against an arithmetic back-end:

  * `Exact`: every intermediate is a pair R(v, e).  v is the value in np.longdouble (64-bit mantissa); e bounds |float64 - v| for ANY float64
    evaluation of the same formula -- any summation order, with or without fma.  First-order rules, u = 2^-53:
      add / sub / mul / div       the standard propagation + u |result|
      sums and dot products       sum e_i + gamma_{n-1} sum |v_i|   (gamma_n = n u / (1 - n u)); independent of order, so it covers wave,
                                  block and tile reductions and fma chains alike
      sqrt                        min(e / (2 sqrt v), sqrt e) + u sqrt v
      exp, log, pow               the secant over [v - e, v + e] (each is monotone in each argument) + the device library's tested error
                                  (test_device_math_accuracy): exp and log 2 ulp, pow 3 + |y ln x| ulp
      sin, cos                    e (1-Lipschitz) + max(4 ulp, 4e-16)
      abs, max, min, Katsuura's |t - floor(t + 0.5)|    1-Lipschitz: e passes through
      jumps                       Step-Ellipsoid's floor and its |z| > 0.5 switch, the noise threshold: a candidate whose exact decision
                                  quantity lies within its own e of the edge is AMBIGUOUS; its allowance covers both branch values and it
                                  is counted apart
    Decimal literals of the formula (0.1, 0.49, 2 pi, ...) are exact reals, charged their float64 rounding.  Derived tables that desc() ships
    in float64 (10^(6i/(D-1)), 100^lin, the T_asy beta ramp, Lunacek's s and mu1, Weierstrass f0, ...) are recomputed in longdouble from their
    formula and charged |table - exact|.  The problem's own data (shift, maps, bias, Gallagher peaks) are exact inputs.
  * `F64`: plain numpy float64 with the same formula, optionally with one deliberate defect (the teeth of the checker, tests/test_bbob_exact.py).

Kernel reformulations covered by the model, each in the stage that has it (mbx_device.hpp):
  * T_osz: the kernels evaluate exp(t) ** 0.1 as exp(0.1 t) and L / 0.1 as a corrected product; the model is written in the kernels' form
    (the rounding of 0.1 t, up to u |0.1 t| relative, exceeds what the reference's pow adds) plus one extra u |y| for the quotient.
  * Gallagher: z_k = R x - R y_k (R y_k precomputed at upload) instead of R (x - y_k): both products are charged (gamma_D (|R| |x| + |R| |y_k|)),
    which covers the reference's form too.  The winning peak is chosen on a logarithmic key with its own error; every peak whose key can tie the
    best one's is a competitor and its value gap is charged.
  * Weierstrass: cos(3^k b) by complex cubing of (cos b, sin b).  Angle and radius errors triple at every cube, so term k is charged
    3^k (e_b + u |b| + 48 u) -- the same 3^k growth as the reference's own rounding of the argument 3^k b (u 3^k |b|); 48 u covers the initial
    pair's 4 ulp errors and the roundings of the cubes.
The cost the kernels store is f - optimum (row_post), with optimum = f(xopt) = bias: the exact target is f - bias, and the bias addition and
subtraction are charged as roundings at |f + bias|.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, f'np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the exact BBOB objectives need >= 63'

U = 2.0 ** -53
PI = 4 * np.arctan(LD(1))
TWO_PI = 2 * PI
KTWO_PI = 6.283185307179586          # the kernels' and numpy's float64 2 pi
NOISE_NONE, NOISE_GAUSS, NOISE_UNIFORM, NOISE_CAUCHY = 0, 1, 2, 3
BH_KINDS = (1, 2, 7, 8, 9, 10, 14, 17, 18, 19, 21, 22)      # kinds that add pen_coef * pen(x) (the boundaryHandling term)


def gamma(n):
    return n * U / (1 - n * U)


def _f(v):
    return np.asarray(v, dtype=LD).astype(np.float64)


def _lit(s):
    """(exact real, its float64 rounding) of a decimal literal or a float."""
    if isinstance(s, str):
        ex = LD(s)
        return ex, float(s)
    return LD(s), float(s)


# ================================================================================================ the (value, bound) pair
class R:
    __array_ufunc__ = None                      # numpy operands defer to R's reflected operators

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def lift(a):
        return a if isinstance(a, R) else R(a)

    def __getitem__(self, k):
        return R(self.v[k], self.e[k])

    @property
    def shape(self):
        return self.v.shape

    def _rnd(self):
        return U * np.abs(_f(self.v))

    def __add__(self, o):
        o = R.lift(o)
        r = R(self.v + o.v, 0.)
        r.e = self.e + o.e + r._rnd()
        return r
    __radd__ = __add__

    def __sub__(self, o):
        o = R.lift(o)
        r = R(self.v - o.v, 0.)
        r.e = self.e + o.e + r._rnd()
        return r

    def __rsub__(self, o):
        return R.lift(o) - self

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = R.lift(o)
        r = R(self.v * o.v, 0.)
        r.e = np.abs(_f(self.v)) * o.e + np.abs(_f(o.v)) * self.e + self.e * o.e + r._rnd()
        return r
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R.lift(o)
        r = R(self.v / o.v, 0.)
        den = np.abs(_f(o.v)) - o.e
        with np.errstate(divide='ignore', invalid='ignore'):
            r.e = np.where(den > 0, (self.e + np.abs(_f(r.v)) * o.e) / np.where(den > 0, den, 1.), np.inf) + r._rnd()
        return r

    def __rtruediv__(self, o):
        return R.lift(o) / self


def _where(c, a, b):
    a, b = R.lift(a), R.lift(b)
    return R(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def _secant(fn, x, xe, lo_clip=None):
    """max |fn(x') - fn(x)| over x' in [x - xe, x + xe] for a monotone fn (in longdouble)."""
    lo = x - xe.astype(LD)
    if lo_clip is not None:
        lo = np.maximum(lo, lo_clip)
    hi = x + xe.astype(LD)
    with np.errstate(all='ignore'):
        f0 = fn(x)
        d = np.maximum(np.abs(fn(lo) - f0), np.abs(fn(hi) - f0))
    return np.where(np.isfinite(d), _f(d), np.inf)


# ================================================================================================ back-ends
class Exact:
    """Longdouble values with running error bounds."""
    exact = True

    def lit(self, s):
        ex, f = _lit(s)
        return R(ex, abs(float(LD(f) - ex)))

    def table(self, exact, f64):
        """A table desc() ships in float64 whose exact value is `exact` (longdouble): charged |f64 - exact|."""
        exact = np.asarray(exact, dtype=LD)
        return R(exact, _f(np.abs(np.asarray(f64, dtype=LD) - exact)))

    def data(self, a):
        return R(np.asarray(a, dtype=np.float64).astype(LD))

    def x(self, X):
        if isinstance(X, R):                    # a position known to (value, bound): its bound propagates
            return X
        return R(np.asarray(X, dtype=np.float64).astype(LD))

    def dot(self, M, y):
        """y [.., D] -> M y along the last axis (sr_func's matmul): a D-term dot product per output."""
        M = R.lift(M)
        D = M.v.shape[-1]
        Mv, Ma = M.v, np.abs(_f(M.v))
        v = np.matmul(y.v, Mv.T)
        ya = np.abs(_f(y.v))
        e = np.matmul(y.e, Ma.T) + np.matmul(ya, M.e.T) + gamma(D) * np.matmul(ya, Ma.T)
        return R(v, e)

    def sum(self, x, axis=-1):
        n = x.v.shape[axis]
        return R(x.v.sum(axis), x.e.sum(axis) + gamma(max(n - 1, 0)) * np.abs(_f(x.v)).sum(axis))

    def prod(self, x):
        r = x[..., 0]
        for d in range(1, x.shape[-1]):
            r = r * x[..., d]
        return r

    def sqrt(self, x):
        v = np.sqrt(np.maximum(x.v, 0))
        vf = _f(v)
        with np.errstate(divide='ignore', invalid='ignore'):
            lin = np.where(vf > 0, x.e / (2 * np.where(vf > 0, vf, 1.)), np.inf)
        return R(v, np.minimum(lin, np.sqrt(x.e)) + U * vf)

    def exp(self, x):
        v = np.exp(x.v)
        return R(v, _secant(np.exp, x.v, x.e) + 4 * U * np.abs(_f(v)))

    def log(self, x):
        v = np.log(x.v)
        return R(v, _secant(np.log, x.v, x.e, LD(0)) + 4 * U * np.abs(_f(v)))

    def _trig(self, fn, x):
        v = fn(x.v)
        return R(v, x.e + np.maximum(8 * U * np.abs(_f(v)), 4e-16))

    def sin(self, x):
        return self._trig(np.sin, x)

    def cos(self, x):
        return self._trig(np.cos, x)

    def pow(self, x, y):
        """x ** y for x >= 0 (the kernels' pow_fast / numpy power)."""
        y = R.lift(y)
        xv, yv = x.v, y.v
        with np.errstate(all='ignore'):
            v = np.power(xv, yv)
            d = np.zeros(np.broadcast(xv, yv).shape, dtype=LD)
            xl = np.maximum(xv - x.e.astype(LD), 0)
            for xs in (xl, xv + x.e.astype(LD)):
                for ys in (yv - y.e.astype(LD), yv + y.e.astype(LD)):
                    d = np.maximum(d, np.abs(np.power(xs, ys) - v))
            dev = (3 + np.abs(_f(yv * np.log(np.where(xv > 0, xv, 1))))) * 2 * U * np.abs(_f(v))
        d = np.where(np.isfinite(d), _f(d), np.inf)
        return R(v, d + dev)

    def abs(self, x):
        return R(np.abs(x.v), x.e)

    def maximum(self, a, b):
        a, b = R.lift(a), R.lift(b)
        return R(np.maximum(a.v, b.v), np.maximum(a.e, b.e))

    def minimum(self, a, b):
        a, b = R.lift(a), R.lift(b)
        return R(np.minimum(a.v, b.v), np.maximum(a.e, b.e))

    def sign(self, x):
        return np.sign(x.v)

    def value(self, x):
        return x.v

    # -- stages with a decision ------------------------------------------------------------------
    def osc(self, x):
        """T_osz in the kernels' form (mbx_device.hpp osc1).  Where e >= |x| / 2 the sign and the logarithm are not resolved: there
        |T_osz(x')| <= 1.11 |x'| (the exponent's oscillation is at most 0.098), so the bound is 1.11 (|x| + e) + |T_osz(x)|."""
        pos = x.v > 0
        safe = x.v != 0
        ax = R(np.where(safe, np.abs(x.v), 1), np.where(safe, x.e, 0.))
        r = _osc_body(self, ax, pos)
        r = R(np.where(pos, r.v, -r.v), r.e)
        r.v = np.where(safe, r.v, 0)
        wide = (x.e >= np.abs(_f(x.v)) / 2)
        r.e = np.where(wide, 1.11 * (np.abs(_f(x.v)) + x.e) + np.abs(_f(r.v)), r.e)
        return r

    def asy(self, x, beta):
        """T_asy: x ** (1 + beta sqrt(x)) for x > 0, else x.  Where the sign is not resolved, both branches are bounded by
        max(|x| + e, (|x| + e) ** (1 + beta sqrt(|x| + e)))."""
        pos = x.v > 0
        xs = R(np.where(pos, x.v, 1), np.where(pos, x.e, 0.))
        p = self.pow(xs, 1 + beta * self.sqrt(xs))
        r = _where(pos, p, x)
        wide = x.e >= np.abs(_f(x.v))
        t = np.abs(_f(x.v)) + x.e
        bmax = np.abs(_f(beta.v)) + beta.e
        with np.errstate(all='ignore'):
            big = np.maximum(t, np.power(t, 1 + bmax * np.sqrt(t)))
        r.e = np.where(wide, big + np.abs(_f(r.v)), r.e)
        return r

    def scale_pos(self, z, sgn, lam):
        """z * lam where z * sgn > 0, else z (Buche-Rastrigin's odd-index boost, the attractive sector): continuous at 0."""
        hit = z.v * sgn > 0
        r = _where(hit, z * lam, z)
        wide = z.e >= np.abs(_f(z.v))
        r.e = np.where(wide, float(lam) * (np.abs(_f(z.v)) + z.e) + np.abs(_f(r.v)), r.e)
        return r

    def katsuura_frac(self, a):
        """|a - floor(a + 0.5)|: the distance to the nearest integer, 1-Lipschitz; the rounding of a + 0.5 only matters at a half-integer,
        where both integers are 0.5 away (+ u)."""
        return R(np.abs(a.v - np.floor(a.v + LD(0.5))), a.e + U)


def _osc_body(ops, ax, pos):
    L = ops.log(ax)
    y = L / ops.lit('0.1')
    if ops.exact:
        y.e = y.e + U * np.abs(_f(y.v))               # the kernels' corrected product L * 10 (div_by_tenth)
    c1 = ops.sel(pos, '1.0', '0.55')
    c2 = ops.sel(pos, '0.79', '0.31')
    t = y + ops.lit('0.49') * (ops.sin(c1 * y) + ops.sin(c2 * y))
    return ops.exp(ops.lit('0.1') * t)


def _exact_sel(self, c, a, b):
    A, B = self.lit(a), self.lit(b)
    return _where(c, A, B)


Exact.sel = _exact_sel


class F64:
    """numpy float64 evaluation of the same formula.  `defect`: None, 'maps32' (maps and shift rounded to float32), 'trans' (exp off by a factor
    1 + 2^-40), 'acc32' (the matvec accumulates in float32), 'osz32' (the T_osz constants in float32)."""
    exact = False

    def __init__(self, defect=None):
        self.defect = defect

    def lit(self, s):
        return float(s)

    def sel(self, c, a, b):
        cast = np.float32 if self.defect == 'osz32' else float
        return np.where(c, float(cast(float(a))), float(cast(float(b))))

    def table(self, exact, f64):
        return np.asarray(f64, dtype=np.float64)

    def data(self, a):
        a = np.asarray(a, dtype=np.float64)
        return a.astype(np.float32).astype(np.float64) if self.defect == 'maps32' else a

    def x(self, X):
        return np.asarray(X, dtype=np.float64)

    def dot(self, M, y):
        if self.defect == 'acc32':
            acc = np.zeros(y.shape[:-1] + (M.shape[0],), dtype=np.float32)
            for k in range(M.shape[1]):
                acc = (acc + (y[..., k, None] * M[:, k]).astype(np.float32)).astype(np.float32)
            return acc.astype(np.float64)
        out = np.zeros(y.shape[:-1] + (M.shape[0],))
        for k in range(M.shape[1]):
            out = out + y[..., k, None] * M[:, k]
        return out

    def sum(self, x, axis=-1):
        return np.sum(x, axis)

    def prod(self, x):
        return np.prod(x, -1)

    sqrt = staticmethod(np.sqrt)
    log = staticmethod(np.log)
    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)
    abs = staticmethod(np.abs)
    maximum = staticmethod(np.maximum)
    minimum = staticmethod(np.minimum)
    sign = staticmethod(np.sign)

    def exp(self, x):
        r = np.exp(x)
        return r * (1 + 2.0 ** -40) if self.defect == 'trans' else r

    def pow(self, x, y):
        with np.errstate(all='ignore'):
            return np.power(x, y)

    def value(self, x):
        return x

    def osc(self, x):
        pos = x > 0
        ax = np.where(x != 0, np.abs(x), 1.)
        o = 0.1 if self.defect != 'osz32' else float(np.float32(0.1))
        L = np.log(ax)
        y = L / o
        c1, c2 = self.sel(pos, '1.0', '0.55'), self.sel(pos, '0.79', '0.31')
        c49 = 0.49 if self.defect != 'osz32' else float(np.float32(0.49))
        r = self.exp(o * (y + c49 * (np.sin(c1 * y) + np.sin(c2 * y))))
        return np.where(x == 0, 0., np.where(pos, r, -r))

    def asy(self, x, beta):
        with np.errstate(all='ignore'):
            return np.where(x > 0, np.power(np.where(x > 0, x, 1.), 1 + beta * np.sqrt(np.where(x > 0, x, 0.))), x)

    def scale_pos(self, z, sgn, lam):
        return np.where(z * sgn > 0, z * lam, z)

    def katsuura_frac(self, a):
        return np.abs(a - np.floor(a + 0.5))


# ================================================================================================ derived tables (exact | float64)
def tables(desc):
    """The problem's inputs as (exact longdouble, float64) pairs: data tables are exact; derived ones are recomputed from their formula."""
    d = desc
    D, k = int(d['dim']), int(d['kind'])
    i = np.arange(D).astype(LD)
    lin = i / (D - 1)
    t = {}

    def put(name, exact):
        if d.get(name) is not None:
            t[name] = (np.asarray(exact, dtype=LD), np.asarray(d[name], dtype=np.float64))
    sh = np.asarray(d['dshift'], dtype=np.float64)
    sgn = np.sign(sh).astype(LD)
    if k == 2:
        put('v0', np.power(LD(10), 6 * i / (D - 1)))
    elif k in (3, 15):
        put('v0', np.power(LD(10), lin / 2))
        put('v1', LD('0.2') * lin)
    elif k == 4:
        put('v0', np.power(LD(10), lin / 2))
    elif k == 5:
        put('v0', sgn * np.power(LD(10), lin))
        put('v1', LD(d['ub']) * np.power(LD(10), lin))
    elif k == 7:
        put('v0', np.power(LD(100), lin))
    elif k == 10:
        cond = LD(10) ** 6 if int(d['func_id']) == 10 else LD(10) ** 4
        put('v0', np.power(cond, lin))
    elif k in (12, 17, 18):
        put('v1', LD('0.5') * lin)
    elif k == 14:
        put('v0', 2 + 4 * i / max(1, D - 1))
    elif k == 20:
        put('v0', np.power(LD(10), lin / 2))
        put('v1', 2 * np.abs(sh).astype(LD))
        put('v2', 2 * sgn)
    elif k == 24:
        put('v0', 2 * sgn)
    for name in ('dshift', 'm1', 'm2', 'py', 'pc', 'pw'):
        if d.get(name) is not None:
            a = np.asarray(d[name], dtype=np.float64)
            t[name] = (a.astype(LD), a)
    s = np.asarray(d['s'], dtype=np.float64)
    sx = s.astype(LD)
    if k == 8:
        sx[0] = max(LD(1), np.sqrt(LD(D)) / 8)
    elif k == 16:
        sx[0] = -(2 - LD(2) ** -11)                      # sum_k 0.5^k cos(pi 3^k): 3^k is odd
    elif k == 24:
        ss = 1 - 1 / (2 * np.sqrt(LD(D) + 20) - LD('8.2'))
        mu0 = LD('2.5') / 5 * LD(d['ub'])
        sx[0], sx[1], sx[2] = mu0, ss, -np.sqrt((mu0 ** 2 - 1) / ss)
    t['s'] = (sx, s)
    return t


# ================================================================================================ the formula
def _pen(ops, x, ub):
    q = ops.maximum(0., ops.abs(x) - ub)
    return ops.sum(q * q)


def _matvec(ops, T, name, y):
    return ops.dot(ops.data(T[name][1]) if not ops.exact else R(T[name][0]), y)


def _core(ops, desc, X):
    """f(x) - bias for every row of X (the value the kernels store as cost, before noise), in the back-end `ops`."""
    d = desc
    T = tables(d)
    D, k = int(d['dim']), int(d['kind'])
    ub = float(d['ub'])
    x = ops.x(X)

    def tab(name):
        ex, f = T[name]
        return ops.table(ex, f) if ops.exact else ops.table(ex, f)

    def data(name):
        return R(T[name][0]) if ops.exact else ops.data(T[name][1])

    def shifted():
        return x - data('dshift')

    def M(name, y):
        return ops.dot(data(name), y)

    s_ = tab('s')

    def s(j):
        return s_[j] if ops.exact else s_[j]

    pen = None
    if k == 1:
        z = M('m1', shifted())
        f = ops.sum(z * z)
    elif k in (2, 10):
        o = ops.osc(M('m1', shifted()))
        f = ops.sum(tab('v0') * (o * o))
    elif k in (3, 4, 15):
        z = ops.osc(M('m1', shifted()))
        if k == 3:
            z = tab('v0') * ops.asy(z, tab('v1'))
        elif k == 4:
            ev = (np.arange(D) % 2 == 0).astype(np.float64)
            z = ops.scale_pos(z, ev, 10.) * tab('v0')
        else:
            z = M('m2', ops.asy(z, tab('v1')))
        sc = ops.sum(ops.cos(_two_pi(ops) * z))
        f = ops.lit('10') * (D - sc) + ops.sum(z * z)
        if k == 4:
            f = f + ops.lit('100') * _pen(ops, x, ub)
    elif k == 5:
        if isinstance(X, R):
            raise NotImplementedError('Linear Slope takes float64 positions only (its box clip is decided on X itself)')
        sh = np.asarray(d['dshift'], dtype=np.float64)
        v0, v1 = tab('v0'), tab('v1')
        X64 = np.asarray(X, dtype=np.float64)
        out = (X64.astype(LD) * sh.astype(LD)) > LD(ub) ** 2
        zi_v = np.where(out, np.sign(X64) * ub, X64)
        zi = ops.x(zi_v)
        if ops.exact:
            edge = np.abs(X64.astype(LD) * sh.astype(LD) - LD(ub) ** 2) <= 4 * U * ub * ub
            zi.e = np.where(edge, np.abs(X64 - np.sign(X64) * ub), 0.)
        else:
            zi = np.where(X64 * sh > ub * ub, np.sign(X64) * ub, X64)
        f = ops.sum(v1 - zi * v0)
    elif k == 6:
        sh = np.asarray(d['dshift'], dtype=np.float64)
        z = ops.scale_pos(M('m1', shifted()), np.sign(sh), 100.)
        f = ops.pow(ops.osc(ops.sum(z * z)), ops.lit('0.9'))
    elif k == 7:
        return _step_ellipsoid(ops, d, T, x, tab, data)
    elif k in (8, 9):
        z = M('m1', shifted())
        z = s(0) * z + 1. if k == 8 else z + ops.lit('0.5')
        a = z[..., :-1] * z[..., :-1] - z[..., 1:]
        b = z[..., :-1] - 1.
        f = ops.sum(ops.lit('100') * (a * a) + b * b)
    elif k == 11:
        o = ops.osc(M('m1', shifted()))
        o2 = o * o
        f = ops.lit('1e6') * o2[..., 0] + ops.sum(o2[..., 1:])
    elif k == 12:
        z = M('m1', ops.asy(M('m1', shifted()), tab('v1')))
        f = z[..., 0] * z[..., 0] + ops.sum(ops.lit('1e6') * (z[..., 1:] * z[..., 1:]))
    elif k == 13:
        z = M('m1', shifted())
        f = z[..., 0] * z[..., 0] + ops.lit('100') * ops.sqrt(ops.sum(z[..., 1:] * z[..., 1:]))
    elif k == 14:
        z = M('m1', shifted())
        f = ops.pow(ops.sum(ops.pow(ops.abs(z), tab('v0'))), ops.lit('0.5'))
    elif k == 16:
        z = M('m2', ops.osc(M('m1', shifted())))
        acc = ops.sum(_weierstrass(ops, z))
        g = acc / D - s(1 - 1)
        f = ops.lit('10') * ops.pow3(g) + (ops.lit('10') / D) * _pen(ops, x, ub)
    elif k in (17, 18):
        z = M('m2', ops.asy(M('m1', shifted()), tab('v1')))
        sq = ops.sqrt(z[..., :-1] * z[..., :-1] + z[..., 1:] * z[..., 1:])
        w = ops.sin(ops.lit('50') * ops.pow(sq, ops.lit('0.2')))
        acc = ops.sum(ops.sqrt(sq) * (w * w + 1.))
        g = (ops.lit('1') / (D - 1)) * acc
        f = g * g
    elif k == 19:
        z = M('m1', shifted()) + ops.lit('0.5')
        a = z[..., :-1] * z[..., :-1] - z[..., 1:]
        b = 1. - z[..., :-1]
        sv = ops.lit('100') * (a * a) + b * b
        acc = ops.sum(sv / ops.lit('4000') - ops.cos(sv))
        f = s(0) + s(0) * acc / (D - 1.)
    elif k == 20:
        v0, v1, v2 = tab('v0'), tab('v1'), tab('v2')
        t = v2 * x
        zi = t[..., 1:] + ops.lit('0.25') * (t[..., :-1] - v1[:-1])
        zi = _concat(ops, t[..., :1], zi)
        z = ops.lit('100') * (v0 * (zi - v1) + v1)
        acc = ops.sum(z * ops.sin(ops.sqrt(ops.abs(z))))
        q = ops.maximum(0., ops.abs(z / ops.lit('100')) - ub)
        f = (ops.lit('4.189828872724339') - ops.lit('0.01') * (acc / D)) + ops.lit('100') * ops.sum(q * q)
    elif k in (21, 22):
        best = _gallagher(ops, d, T, x)
        o = ops.osc(ops.lit('10') - best)
        f = o * o
    elif k == 23:
        z = M('m1', shifted())
        kexp = ops.lit('10') / ops.pow(ops.lit(float(D)), ops.lit('1.2'))
        temp = None
        for j in range(1, 33):
            a = z * float(2.0 ** j)
            term = ops.katsuura_frac(a) * float(2.0 ** -j)
            temp = term if temp is None else temp + term
        ii = np.arange(1, D + 1).astype(np.float64)
        res = ops.prod(ops.pow(1. + ii * temp, kexp))
        tmp = ops.lit('10') / D / D
        f = (res * tmp - tmp) + _pen(ops, x, ub)
    elif k == 24:
        v0 = tab('v0')
        mu0, sc_, mu1 = s(0), s(1), s(2)
        xh = v0 * x
        a = ops.sum((xh - mu0) * (xh - mu0))
        b = ops.sum((xh - mu1) * (xh - mu1))
        z = M('m1', xh - mu0)
        sc = ops.sum(ops.cos(_two_pi(ops) * z))
        f = ops.minimum(a, D + sc_ * b) + ops.lit('10') * (D - sc) + ops.lit('1e4') * _pen(ops, x, ub)
    else:
        raise ValueError(f'kind {k}')
    if k in BH_KINDS and float(d['pen_coef']) != 0.:
        f = f + ops.lit(float(d['pen_coef'])) * _pen(ops, x, ub)
    return _through_bias(ops, f, float(d['bias']))


def _two_pi(ops):
    return R(TWO_PI, abs(float(LD(KTWO_PI) - TWO_PI))) if ops.exact else KTWO_PI


def _concat(ops, a, b):
    if ops.exact:
        return R(np.concatenate([a.v, b.v], -1), np.concatenate([a.e, b.e], -1))
    return np.concatenate([a, b], -1)


def _through_bias(ops, f, bias):
    """(f + bias [+ ...]) - optimum with optimum = bias: the value stays f, the two roundings are charged at |f + bias| (twice, for any
    placement of bias among the final additions) and |f|."""
    if ops.exact:
        return R(f.v, f.e + 2 * U * np.abs(_f(f.v) + bias) + U * np.abs(_f(f.v)))
    return (f + bias) - bias


def _exact_pow3(self, g):
    return self.pow(g, 3.) if not self.exact else _pow_odd3(self, g)


def _pow_odd3(ops, g):
    """g ** 3 for any sign (pow of a negative base with an odd integer exponent): |g|^3 with the sign; the pow error taken at |g|."""
    a = ops.pow(ops.abs(g), 3.)
    sg = np.sign(g.v)
    return R(sg * a.v, a.e + np.where(g.e >= np.abs(_f(g.v)), 8 * (np.abs(_f(g.v)) + g.e) ** 3, 0.))


Exact.pow3 = _exact_pow3
F64.pow3 = lambda self, g: np.power(g, 3.)


def _weierstrass(ops, z):
    """sum_k 0.5^k cos(3^k 2 pi (z + 0.5)), k < 12, per coordinate (see the module docstring for the kernels' complex-cubing form)."""
    if not ops.exact:
        b = KTWO_PI * (z + 0.5)
        return sum(0.5 ** kk * np.cos(b * 3.0 ** kk) for kk in range(12))
    zp = z + ops.lit('0.5')
    b = _two_pi(ops) * zp
    v = sum(LD(0.5) ** kk * np.cos(LD(3) ** kk * b.v) for kk in range(12))
    bf = np.abs(_f(b.v))
    e = sum(0.5 ** kk * (3.0 ** kk * (b.e + U * bf + 48 * U)) for kk in range(12))
    mag = sum(0.5 ** kk * np.abs(_f(np.cos(LD(3) ** kk * b.v))) for kk in range(12))
    return R(v, e + gamma(12) * mag + 8 * U)


def _step_ellipsoid(ops, d, T, x, tab, data):
    """F7.  z_hat = M1 (x - shift); z~ = floor(0.5 + z_hat) where |z_hat| > 0.5, else floor(0.5 + 10 z_hat) / 10; z = M2 z~;
    f = 0.1 max(|z_hat_0| / 1e4, sum 100^lin z^2) + pen.  In the exact back-end every coordinate whose decision quantity (|z_hat| - 0.5,
    or the distance of 0.5 + z_hat, 0.5 + 10 z_hat to an integer) is within its error of the edge is ambiguous: the allowance covers every
    combination of its possible z~ values."""
    D = int(d['dim'])
    ub = float(d['ub'])
    zh = ops.dot(data('m1'), x - data('dshift'))
    v0 = tab('v0')
    pen = ops.lit(float(d['pen_coef'])) * _pen(ops, x, ub) if float(d['pen_coef']) else 0.
    if not ops.exact:
        zt = np.where(np.abs(zh) > 0.5, np.floor(0.5 + zh), np.floor(0.5 + 10. * zh) / 10.)
        z = ops.dot(data('m2'), zt)
        f = 0.1 * np.maximum(np.abs(zh[..., 0]) / 1e4, np.sum(v0 * (z * z), -1)) + pen
        return _through_bias(ops, f, float(d['bias']))
    hv = zh.v
    big = np.abs(hv) > 0.5
    tA = hv + LD(0.5)
    eA = zh.e + U * np.abs(_f(tA))
    tB = 10 * hv + LD(0.5)
    eB = 10 * zh.e + U * 10 * np.abs(_f(hv)) + U * np.abs(_f(tB))
    zt = np.where(big, np.floor(tA), np.floor(tB) / 10)
    zte = np.where(big, 0., U * np.abs(_f(zt)))
    amb_sw = np.abs(np.abs(hv) - LD(0.5)) <= zh.e
    ambA = (big | amb_sw) & (np.abs(tA - np.round(tA)) <= eA)
    ambB = (~big | amb_sw) & (np.abs(tB - np.round(tB)) <= eB)
    amb = amb_sw | ambA | ambB
    rows, cols = np.nonzero(amb)
    m2 = T['m2'][0]
    v0e = T['v0'][0]

    def sval(ztr):
        zz = ztr @ m2.T
        return (v0e * zz * zz).sum(-1)
    s_ex = sval(zt)
    # the main path, with its rounding bounds
    zr = ops.dot(R(m2), R(zt, zte))
    sr = ops.sum(v0 * (zr * zr))
    a = ops.abs(zh[..., 0]) / ops.lit('1e4')
    f = ops.lit('0.1') * ops.maximum(a, sr) + pen
    n_amb = np.zeros(hv.shape[0], dtype=np.int64)
    extra = np.zeros(hv.shape[0])
    for r in np.unique(rows):
        cs = cols[rows == r]
        n_amb[r] = len(cs)
        options = []
        for c in cs:
            keep = set()
            if amb_sw[r, c] or big[r, c]:
                keep |= {np.floor(tA[r, c] - LD(eA[r, c])), np.floor(tA[r, c] + LD(eA[r, c]))}
            if amb_sw[r, c] or not big[r, c]:
                keep |= {np.floor(tB[r, c] - LD(eB[r, c])) / 10, np.floor(tB[r, c] + LD(eB[r, c])) / 10}
            options.append(sorted(keep))
        worst = LD(0)
        base = LD('0.1') * max(abs(hv[r, 0]) / LD(10000), s_ex[r])
        combos = [[]]
        for opt in options[:10]:
            combos = [cmb + [o] for cmb in combos for o in opt]
        for cmb in combos:
            z2 = zt[r].copy()
            for c, val in zip(cs[:10], cmb):
                z2[c] = val
            alt = LD('0.1') * max(abs(hv[r, 0]) / LD(10000), sval(z2[None])[0])
            worst = max(worst, abs(alt - base))
        extra[r] = float(worst) * (1 + 1e-12) + 0.1 * (np.abs(_f(sr.v[r])) + sr.e[r]) * 1e-12
    f = R(f.v, f.e + extra)
    out = _through_bias(ops, f, float(d['bias']))
    out._amb = n_amb
    return out


def _gallagher(ops, d, T, x):
    """max_k w_k exp(-1/(2D) sum_d C_kd z_kd^2), z_k = R (x - y_k) (see the module docstring for the reformulation and the peak choice)."""
    D, npk = int(d['dim']), int(d['n_peaks'])
    Rm = T['m1'][0]
    Y = T['py'][0].reshape(npk, D)
    C = T['pc'][0].reshape(npk, D)
    W = T['pw'][0]
    if not ops.exact:
        Rf, Yf, Cf, Wf = (np.asarray(T[n][1], dtype=np.float64) for n in ('m1', 'py', 'pc', 'pw'))
        Rf = ops.data(Rf)
        z = ops.dot(Rf, x[..., None, :] - Yf.reshape(npk, D))
        acc = np.sum(Cf.reshape(npk, D) * (z * z), -1)
        return np.max(Wf * ops.exp((-0.5 / D) * acc), -1)
    xv = x.v
    zx = ops.dot(R(Rm), x)                                                    # R x
    ry = ops.dot(R(Rm), R(Y))                                                 # R y_k
    zv = zx.v[..., None, :] - ry.v[None]
    ze = zx.e[..., None, :] + ry.e[None] + U * np.abs(_f(zv))
    z = R(zv, ze)
    acc = ops.sum(R(C) * (z * z))                                             # [m, npk]
    cexp = ops.lit('-0.5') / D
    ex = ops.exp(cexp * acc)
    val = R(W) * ex
    kbest = np.argmax(val.v, -1)
    rows = np.arange(val.v.shape[0])
    best = val.v[rows, kbest]
    # key_k = log w_k + cexp acc_k: its error (log w_k rounded on the host, 2 ulp; the fma chain; the product; the sum)
    key = np.log(W)[None] + cexp.v * acc.v
    ekey = (4 * U * np.abs(_f(np.log(W))))[None] + np.abs(float(cexp.v)) * acc.e + cexp.e * np.abs(_f(acc.v)) + 2 * U * np.abs(_f(key))
    kb = key[rows, kbest][:, None]
    comp = key >= kb - (ekey[rows, kbest][:, None] + ekey).astype(LD)
    gap = np.where(comp, val.e + _f(best[:, None] - val.v), 0.)
    return R(best, gap.max(-1))


def _noise(ops, cost, desc, draws):
    """NoisyProblem.noisy (bbob.py:108-146) on the cost f - optimum, then + optimum + 1.01e-8 - optimum (row_post).
    draws [3, m]: the model's (a, b, c) per row.  -> (R, ambiguous rows) in the exact back-end."""
    nk = int(desc['noise_kind'])
    if nk == NOISE_NONE:
        return cost, np.zeros(cost.shape[0] if ops.exact else len(cost), dtype=bool)
    a_, b_, c_ = (np.asarray(draws[j], dtype=np.float64) for j in range(3))
    al, be, D = float(desc['noise_a']), float(desc['noise_b']), int(desc['dim'])
    fu = cost
    if nk == NOISE_GAUSS:
        fn = fu * ops.exp(ops.lit(al) * ops.x(a_))
    elif nk == NOISE_UNIFORM:
        base = ops.lit('1e9') / (fu + ops.lit('1e-99'))
        expo = ops.lit(al) * (ops.lit('0.49') + ops.lit('1') / D) * ops.x(b_)
        if ops.exact:
            base = R(np.maximum(base.v, LD(0)), base.e)
        fn = fu * ops.pow(ops.x(a_), ops.lit(be)) * ops.maximum(1., ops.pow(base, expo))
    else:
        hit = (a_ < be).astype(np.float64)
        fn = fu + ops.lit(al) * ops.maximum(0., ops.lit('1e3') + ops.x(hit) * ops.x(b_) / (ops.abs(ops.x(c_)) + ops.lit('1e-199')))
    if not ops.exact:
        bias = float(desc['bias'])
        out = ((fn + bias) + 1.01 * 1e-8) - bias
        return np.where(fu >= 1e-8, out, fu), None
    c = ops.lit('1.01e-8')
    noisy = R(fn.v + c.v, fn.e + c.e + 3 * U * np.abs(_f(fn.v + c.v) + float(desc['bias'])) + U * np.abs(_f(fn.v + c.v)))
    th = LD(1e-8)
    go = fu.v >= th
    amb = np.abs(fu.v - th) <= fu.e
    v = np.where(go, noisy.v, fu.v)
    e = np.where(go, noisy.e, fu.e)
    alt_gap = np.where(go, _f(np.abs(noisy.v - fu.v)) + fu.e, _f(np.abs(noisy.v - fu.v)) + noisy.e)
    e = np.where(amb, np.maximum(e, alt_gap) * (1 + 1e-12), e)
    return R(v, e), amb


# ================================================================================================ public surface
def _desc(problem):
    return problem.desc() if hasattr(problem, 'desc') else problem


def _eval(problem, X, draws=None, ops=None):
    """X: float64 rows, or (Exact back-end only) an R [m, D] of positions known to within X.e: the allowance then covers any float64
    evaluation at any float64 point within that bound."""
    d = _desc(problem)
    if not isinstance(X, R):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    ops = ops or Exact()
    with np.errstate(over='ignore', invalid='ignore'):
        c = _core(ops, d, X)
        amb = getattr(c, '_amb', None)
        if draws is not None and int(d['noise_kind']) != NOISE_NONE:
            c, namb = _noise(ops, c, d, draws)
            if ops.exact:
                amb = (amb if amb is not None else 0) + namb.astype(np.int64)
    if ops.exact and amb is None:
        amb = np.zeros(X.shape[0], dtype=np.int64)
    return c, amb


def exact(problem, X, draws=None):
    """Exact costs f(x) - optimum of the rows of X (longdouble); with `draws` [3, m] the noisy cost of a noisy problem."""
    return _eval(problem, X, draws)[0].v


def allowance(problem, X, draws=None):
    """-> (allow [m] float64, n_ambiguous [m] int, exact [m] longdouble)."""
    c, amb = _eval(problem, X, draws)
    return c.e.copy(), np.asarray(amb, dtype=np.int64), c.v


def float64_eval(problem, X, draws=None, defect=None):
    """The same formula in plain float64 (optionally with one defect, see F64): the cost f - optimum."""
    ops = F64(defect)
    d = _desc(problem)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    with np.errstate(all='ignore'):
        c = _core(ops, d, X)
        if draws is not None and int(d['noise_kind']) != NOISE_NONE:
            c, _ = _noise(ops, c, d, draws)
    return c


def check(problem, X, got, draws=None, label=''):
    allow, namb, ex = allowance(problem, X, draws)
    err = np.abs(np.asarray(got, dtype=LD) - ex).astype(np.float64)
    ratio = err / allow
    bad = np.nonzero(~(ratio <= 1.))[0]
    assert bad.size == 0, (f'{label} {problem}: {bad.size} of {len(ratio)} rows outside the allowance; worst ratio {np.nanmax(ratio):.3g}',
                           [(int(k), float(got[k]), float(ex[k]), float(allow[k]), int(namb[k])) for k in bad[:5]])
    return ratio, namb


# ================================================================================================ adversarial candidates
def _nudge(v, k):
    """v moved by k ulp (k may be negative)."""
    out = np.float64(v)
    for _ in range(abs(int(k))):
        out = np.nextafter(out, np.inf if k > 0 else -np.inf)
    return float(out)


def _solve(M, z):
    """x with M x = z in longdouble (Gaussian elimination with partial pivoting), for a few right-hand sides z [m, D]."""
    A = np.asarray(M, dtype=LD).copy()
    B = np.asarray(z, dtype=LD).T.copy()
    n = A.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], B[[c, p]] = A[[p, c]], B[[p, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c]
        B[c + 1:] -= f[:, None] * B[c]
    X = np.zeros_like(B)
    for c in range(n - 1, -1, -1):
        X[c] = (B[c] - A[c, c + 1:] @ X[c + 1:]) / A[c, c]
    return X.T


def step_edge_points(problem, rs, n=6):
    """F7 candidates with one z_hat component near an edge (+-0.5, k + 0.5, or (k + 0.5) / 10): solved through the inverse map in longdouble,
    rounded, then the coordinate with the largest map entry nudged by up to 16 ulp to bring the component closest to its target.
    -> (X [m, D], component index [m], target [m] longdouble)."""
    d = _desc(problem)
    D = int(d['dim'])
    M = np.asarray(d['m1'], dtype=np.float64).reshape(D, D)
    sh = np.asarray(d['dshift'], dtype=np.float64)
    out, comp, tgt = [], [], []
    edges = [LD(0.5), LD(-0.5), LD(1.5), LD(-2.5), LD(0.25), LD(-0.35)]
    for j in range(n):
        c = int(rs.randint(D))
        e = edges[j % len(edges)]
        zt = rs.uniform(-1.5, 1.5, size=D).astype(LD)
        zt[c] = e + LD(rs.choice([-8, -2, 2, 8])) * LD(2.0 ** -53)
        x = _solve(M.astype(LD), zt[None])[0] + sh.astype(LD)
        if np.any(np.abs(x.astype(np.float64)) > 5):
            continue
        xf = x.astype(np.float64)
        q = int(np.argmax(np.abs(M[c])))
        best = None
        for k in range(-16, 17):
            xx = xf.copy()
            xx[q] = _nudge(xf[q], k)
            zc = (M[c].astype(LD) * (xx.astype(LD) - sh.astype(LD))).sum()
            dist = abs(zc - e)
            if best is None or dist < best[0]:
                best = (dist, xx)
        out.append(best[1]); comp.append(c); tgt.append(e)
    return np.array(out).reshape(-1, D), np.array(comp), np.array(tgt, dtype=LD)


def threshold_rays(problem, rs, n=3):
    """Points on rays from xopt whose exact cost lies at 1e-8, found by bisection in longdouble and rounded, and the float64 neighbours of the
    crossing on both sides (one ulp along the ray's largest coordinate)."""
    d = _desc(problem)
    D = int(d['dim'])
    xo = np.asarray(problem.opt if hasattr(problem, 'opt') else d['dshift'], dtype=np.float64)
    pts = []
    for _ in range(n):
        u = rs.normal(size=D)
        u /= np.linalg.norm(u)
        lo, hi = 0., 1.
        f = lambda t: float(exact(d, (xo + t * u)[None])[0])
        while f(hi) < 1e-8 and hi < 1e3:
            hi *= 2
        if f(hi) < 1e-8:
            continue
        for _ in range(90):
            mid = 0.5 * (lo + hi)
            if f(mid) < 1e-8:
                lo = mid
            else:
                hi = mid
        x = xo + hi * u
        q = int(np.argmax(np.abs(u)))
        for k in (-1, 0, 1):
            xx = x.copy()
            xx[q] = _nudge(x[q], k)
            pts.append(xx)
    return np.array(pts).reshape(-1, D)


def adversarial(problem, rs, n_random=8):
    """Float64 candidates built from the problem's own xopt and maps (see the module docstring of tests/test_bbob_exact.py)."""
    d = _desc(problem)
    D, k = int(d['dim']), int(d['kind'])
    ub = float(d['ub'])
    xo = np.asarray(problem.opt if hasattr(problem, 'opt') else d['dshift'], dtype=np.float64)
    P = [xo.copy()]
    for kk in (1, 4, 64):
        for sgn in (1, -1):
            x = xo.copy()
            c = int(rs.randint(D))
            x[c] = _nudge(x[c], sgn * kk)
            P.append(x)
    P.extend(threshold_rays(d if not hasattr(problem, 'opt') else problem, rs, n=2))
    # box faces: exactly +-5, one ulp outside, far outside (past Schwefel's 500 edge)
    for v in (ub, -ub, np.nextafter(ub, 10.), np.nextafter(-ub, -10.), 600., -1e3, 37.):
        x = rs.uniform(-ub, ub, size=D)
        x[rs.rand(D) < 0.4] = v
        P.append(x)
    # components of z at 0: x = xopt + M1^-1 z with half of z zero
    if d.get('m1') is not None and k not in (5, 20):
        M = np.asarray(d['m1'], dtype=np.float64).reshape(D, D)
        z = rs.uniform(-2, 2, size=(3, D))
        z[:, rs.rand(D) < 0.5] = 0.
        z[2] *= 1e-6
        base = np.zeros(D) if k in (9, 19, 21, 22) else np.asarray(d['dshift'], dtype=np.float64)
        if k in (9, 19):
            base = xo
            z = z
        X = (_solve(M.astype(LD), z) + base.astype(LD)).astype(np.float64)
        P.extend(X[np.all(np.abs(X) < 1e3, 1)])
    if k == 7:
        X, _, _ = step_edge_points(d, rs)
        P.extend(X)
    if k in (21, 22):
        npk = int(d['n_peaks'])
        Y = np.asarray(d['py'], dtype=np.float64).reshape(npk, D)
        w = np.asarray(d['pw'], dtype=np.float64)
        second = 1 + int(np.argmax(w[1:]))
        P.extend([Y[0], Y[second], 0.5 * (Y[0] + Y[second]), Y[rs.randint(npk)]])
    P.extend(rs.uniform(-ub, ub, size=(n_random, D)))
    return np.ascontiguousarray(np.array(P, dtype=np.float64).reshape(-1, D))
