"""Running error bound of a float32 evaluation.  Test infrastructure only; numpy only.

Fe(value, err): `value` is what exact arithmetic gives on the float32 inputs (carried in float64, whose own 2^-53 is far below every bound
here), `err` bounds the distance of a float32 evaluation of the same expression, one IEEE rounding per operation, from `value`.

  a +- b    ea + eb
  a b       |a| eb + |b| ea + ea eb
  a / b     (ea + |a / b| eb) / (|b| - eb),   asserting |b| > 2 eb
  sqrt a    ea / (sqrt(max(a - ea, 0)) + sqrt a);  0 where a = ea = 0
  sin, cos  ea + K_TRIG u   (absolute: the whole allowance of sinf / cosf, their rounding included)

and after every rounded operation err += u |value| + 2^-149, u = 2^-24 (second-order terms u * err are below one part in 10^7 of the
bound and are left out).  No rounding term where the operation is exact: adding an exact 0 (value 0, err 0), multiplying by an exact 0 or
+-1, dividing an exact 0 or dividing by an exact +-1, negation; a product with an exact power of two 2^k adds nothing for k >= 0 and only
the 2^-149 of a result that may become subnormal for k < 0.  Float32 numbers enter with err = 0 (`lift` checks that they are float32 numbers).

`ulps()` is err in units of u |value|, for reports."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
K_TRIG = 2.0          # absolute error allowed to sinf / cosf, in u: a faithfully rounded result in [0.5, 1] is within one ulp = 2 u


def _pow2(v):
    m, _ = np.frexp(np.abs(v))
    return m == 0.5


class Fe:
    __array_priority__ = 1000.0          # ndarray (op) Fe -> Fe.__r(op)__
    __array_ufunc__ = None

    def __init__(self, value, err=None):
        self.value = np.asarray(value, dtype=np.float64)
        self.err = np.zeros_like(self.value) if err is None else np.broadcast_to(np.asarray(err, dtype=np.float64), self.value.shape).copy()
        assert np.all(self.err >= 0) and np.all(np.isfinite(self.value)) and np.all(np.isfinite(self.err))

    # ---- construction, shape
    @staticmethod
    def lift(x):
        if isinstance(x, Fe):
            return x
        a = np.asarray(x)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a.astype(np.float64)), "Fe: an input that is no float32 number"
        return Fe(a.astype(np.float64))

    @property
    def shape(self):
        return self.value.shape

    def __getitem__(self, i):
        return Fe(self.value[i], self.err[i])

    def reshape(self, *s):
        return Fe(self.value.reshape(*s), self.err.reshape(*s))

    def ulps(self):
        return self.err / np.maximum(U * np.abs(self.value), TINY)

    def _zero(self):
        return (self.value == 0) & (self.err == 0)

    def _one(self):
        return (np.abs(self.value) == 1) & (self.err == 0)

    def _p2(self):
        return _pow2(self.value) & (self.err == 0)

    @staticmethod
    def _round(v, e, exact, tiny_only=False):
        return Fe(v, e + np.where(exact, 0.0, np.where(tiny_only, TINY, U * np.abs(v) + TINY)))

    # ---- arithmetic
    def __neg__(self):
        return Fe(-self.value, self.err)

    def __add__(self, o):
        o = Fe.lift(o)
        return Fe._round(self.value + o.value, self.err + o.err, self._zero() | o._zero())

    __radd__ = __add__

    def __sub__(self, o):
        o = Fe.lift(o)
        return Fe._round(self.value - o.value, self.err + o.err, self._zero() | o._zero())

    def __rsub__(self, o):
        return Fe.lift(o).__sub__(self)

    def __mul__(self, o):
        o = Fe.lift(o)
        a, b = np.abs(self.value), np.abs(o.value)
        e = a * o.err + b * self.err + self.err * o.err
        exact = self._zero() | o._zero() | self._one() | o._one()
        up = (self._p2() & (a >= 1)) | (o._p2() & (b >= 1))
        down = (self._p2() | o._p2()) & ~up
        return Fe._round(self.value * o.value, e, exact | up, down)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Fe.lift(o)
        b = np.abs(o.value)
        assert np.all(b > 2 * o.err), "Fe: a divisor that is not well away from 0 (|b| <= 2 eb)"
        v = self.value / o.value
        return Fe._round(v, (self.err + np.abs(v) * o.err) / (b - o.err), self._zero() | o._one())

    def __rtruediv__(self, o):
        return Fe.lift(o).__truediv__(self)

    def sqrt(self):
        assert np.all(self.value >= 0)
        s = np.sqrt(self.value)
        den = np.sqrt(np.maximum(self.value - self.err, 0.0)) + s
        e = np.where(den > 0, self.err / np.where(den > 0, den, 1.0), 0.0)
        assert np.all((den > 0) | (self.err == 0))
        return Fe._round(s, e, self._zero())

    def sin(self):
        return Fe(np.sin(self.value), self.err + K_TRIG * U)

    def cos(self):
        return Fe(np.cos(self.value), self.err + K_TRIG * U)


def stack(xs, axis=-1):
    """a list of Fe, or of arrays, joined along a new axis"""
    if isinstance(xs[0], Fe):
        shp = np.broadcast_shapes(*[x.shape for x in xs])
        return Fe(np.stack([np.broadcast_to(x.value, shp) for x in xs], axis), np.stack([np.broadcast_to(x.err, shp) for x in xs], axis))
    shp = np.broadcast_shapes(*[np.shape(x) for x in xs])
    return np.stack([np.broadcast_to(x, shp) for x in xs], axis)


def concat(xs, axis=-1):
    if isinstance(xs[0], Fe):
        return Fe(np.concatenate([x.value for x in xs], axis), np.concatenate([x.err for x in xs], axis))
    return np.concatenate(xs, axis)


def ratio(got, fe):
    """(worst |got - value| / err, index of it); an element with err = 0 must be met exactly (ratio 0 there, inf otherwise)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - fe.value)
    assert d.shape == fe.err.shape, (d.shape, fe.err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(fe.err > 0, d / fe.err, np.where(d == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    if q.size == 0:
        return 0.0, None
    k = int(np.argmax(q))
    return float(q.reshape(-1)[k]), np.unravel_index(k, q.shape)
