"""Inputs, references and error bases for the stand-alone SH encoder tests
(csrc/shencoder.hip, csrc/sh_basis.h). Plain numpy, no GPU.

Two references of the same 64 polynomials:

* `oracle._sh_values`, the table typed out as the kernel has it, evaluated in
  any number type; a complex step of 2^-80 on one coordinate puts the exact
  Jacobian of the polynomials into the imaginary part (`jacobian`).
* `independent`, the Cartesian definition by recurrence: A_m + i B_m =
  (x + i y)^m, the associated Legendre functions without the (1 - z^2)^(m/2)
  factor by the three-term recurrence in z, the normalisation from
  factorials. It shares no literal with the table.

The bases are the references' own rounding errors (the maximum over each
group of points, per column), never a kernel's output:

  float32 values    oracle float32 against oracle float64
  float32 Jacobian  complex64 step against complex128 step
  float64 (both)    float64 against long double, both with the
                    float32-rounded literals that sh_basis.h multiplies by
"""
import functools
import math
import types

import numpy as np

import oracle

GROUPS = ("unit", "half", "double")
N_UNIT, N_HALF, N_DOUBLE = 300, 150, 150
N = N_UNIT + N_HALF + N_DOUBLE
GROUP_ID = np.repeat(np.arange(3), (N_UNIT, N_HALF, N_DOUBLE))
STEP = 2.0 ** -80
BATCHES = (1, 63, 64, 65, 255, 256, 257, 600)
# rotation of the interleaved case order per batch size: the short batches
# start at different points so that together they cover every special
# direction; from 255 rows on a prefix holds all of them anyway
ROTATION = {1: 0, 63: 0, 64: 63, 65: 127, 255: 0, 256: 1, 257: 2, 600: 0}

assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, \
    "the float64 kernels' reference needs a long double wider than float64 (x86-64)"


def _f32_literal(T):
    return lambda a: T(np.float32(a))


def _random_dirs(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def special_unit():
    """The hand-picked unit directions, float32 [k, 3]."""
    rows = []
    for a in range(3):                                   # the six axes
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]; v[a] = s; rows.append(v)
    for i in (-1, 0, 1):                                 # the 26 lattice directions
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                if (i, j, k) != (0, 0, 0):
                    n = math.sqrt(i * i + j * j + k * k)
                    rows.append([i / n, j / n, k / n])
    ulp = float(np.spacing(np.float32(1.0)))
    rows += [[ulp, 0.0, 1.0], [ulp, 0.0, -1.0], [-ulp, 0.0, 1.0], [-ulp, 0.0, -1.0]]
    for zero in (0.0, -0.0):
        rows += [[zero, 0.6, 0.8], [0.6, zero, 0.8], [0.6, -0.8, zero],        # one component
                 [zero, zero, 1.0], [zero, -1.0, zero], [1.0, zero, zero]]     # two components
    rows.append([1e-40, 0.6, 0.8])                       # a float32 denormal
    rows.append([0.8, -1e-40, -0.6])
    return np.array(rows, dtype=np.float32)


def inputs(seed=0):
    """float32 [N, 3]: the `unit`, `half` and `double` groups in this order
    (GROUP_ID gives each row's group)."""
    rng = np.random.default_rng(seed)
    sp = special_unit()
    unit = np.concatenate([sp, _random_dirs(rng, N_UNIT - len(sp)).astype(np.float32)])
    half = np.concatenate([np.zeros((1, 3), np.float32),
                           (0.5 * _random_dirs(rng, N_HALF - 1)).astype(np.float32)])
    double = (2.0 * _random_dirs(rng, N_DOUBLE)).astype(np.float32)
    out = np.concatenate([unit, half, double])
    assert out.shape == (N, 3) and out.dtype == np.float32
    return out


def order():
    """Row order in which a prefix holds every group: unit, half, double in
    turn, then the remaining unit rows."""
    u = np.arange(N_UNIT)
    h = N_UNIT + np.arange(N_HALF)
    d = N_UNIT + N_HALF + np.arange(N_DOUBLE)
    k = min(N_HALF, N_DOUBLE)
    head = np.stack([u[:k], h[:k], d[:k]], 1).reshape(-1)
    return np.concatenate([head, u[k:]])


def batch_rows(B):
    """Indices into inputs() of the B rows that batch size B uses."""
    return np.roll(order(), -ROTATION[B])[:B]


# ------------------------------------------------------------ the definition

def _dfact(n):
    return float(np.prod(np.arange(n, 0, -2, dtype=np.float64))) if n > 0 else 1.0


def independent(x, y, z, degree):
    """[n, degree^2] real SH by recurrence (float64, or complex128 for a
    complex step). Column l*l + l + m is (-1)^m sqrt2 K_l^m A_m P_l^m(z) and
    column l*l + l - m the same with B_m; column l*l + l is K_l^0 P_l^0(z)."""
    x, y, z = (np.asarray(v) for v in (x, y, z))
    T = np.result_type(x.dtype, np.float64)
    x, y, z = x.astype(T), y.astype(T), z.astype(T)
    L = degree
    A = [np.ones_like(x)]
    Bm = [np.zeros_like(x)]
    for m in range(1, L):
        A.append(x * A[m - 1] - y * Bm[m - 1])
        Bm.append(x * Bm[m - 1] + y * A[m - 1])
    P = {}
    for m in range(L):
        P[m, m] = _dfact(2 * m - 1) * np.ones_like(z)
        if m + 1 < L:
            P[m + 1, m] = (2 * m + 1) * z * P[m, m]
        for l in range(m + 2, L):
            P[l, m] = ((2 * l - 1) * z * P[l - 1, m] - (l + m - 1) * P[l - 2, m]) / (l - m)
    out = np.zeros((x.shape[0], L * L), dtype=T)
    for l in range(L):
        for m in range(l + 1):
            K = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                out[:, l * l + l] = K * P[l, 0]
            else:
                s = (-1) ** m * math.sqrt(2.0) * K
                out[:, l * l + l + m] = s * A[m] * P[l, m]
                out[:, l * l + l - m] = s * Bm[m] * P[l, m]
    return out


def independent_jacobian(pts, degree):
    """[n, 3, degree^2]: complex step over `independent`."""
    v = np.asarray(pts).astype(np.complex128)
    out = np.empty((v.shape[0], 3, degree * degree))
    for d in range(3):
        w = v.copy(); w[:, d] += 1j * STEP
        out[:, d, :] = independent(w[:, 0], w[:, 1], w[:, 2], degree).imag / STEP
    return out


def depends_on(degree=8):
    """[3, degree^2] bool: whether column c depends on x, y, z at all. m = 0
    columns are polynomials in z alone, m = 1 holds A_1 = x and m = -1 holds
    B_1 = y alone; the l = |m| columns do not hold z; column 0 is a constant."""
    dep = np.zeros((3, degree * degree), dtype=bool)
    for l in range(degree):
        for m in range(-l, l + 1):
            c = l * l + l + m
            dep[0, c] = m not in (0, -1)
            dep[1, c] = m not in (0, 1)
            dep[2, c] = abs(m) != l
    return dep


def structural_zero(dtype, kind):
    """Where a base is zero by construction, so the kernel must be exact:
    [64] bool for kind "val", [3, 64] for "jac".

    float32: only the Jacobian entries of a column with respect to a
    coordinate it does not depend on (column 0 among them); everywhere else
    the float32 rounding of a literal already separates the two references.
    float64: in addition whatever is a float32-rounded literal times at most
    one float32 input (or twice one), 48 bits that float64 holds exactly: the
    values of columns 0 to 3 and every Jacobian entry of columns 0 to 8."""
    col = np.arange(64)
    if kind == "val":
        return col < 4 if dtype == "f64" else np.zeros(64, dtype=bool)
    z = ~depends_on(8)
    if dtype == "f64":
        z = z | (col < 9)[None, :]
    return z


# ------------------------------------------------------------- the references

def values(pts, degree, T, const=None):
    """oracle._sh_values on [n, 3] points converted to T."""
    v = np.asarray(pts).astype(T)
    return oracle._sh_values(v[:, 0], v[:, 1], v[:, 2], degree, T, const)


def jacobian(pts, degree, T, const=None):
    """[n, 3, degree^2] Jacobian of the oracle's table by complex step in the
    complex type T: exact for complex128 / clongdouble (up to the rounding of
    that type), the float32 dual-number evaluation for complex64."""
    v = np.asarray(pts).astype(T)
    R = type(T(0).real)
    h = R(STEP)
    out = np.empty((v.shape[0], 3, degree * degree), dtype=R)
    for d in range(3):
        w = v.copy(); w[:, d] += T(1j) * h
        out[:, d, :] = oracle._sh_values(w[:, 0], w[:, 1], w[:, 2], degree, T, const).imag / h
    return out


def _group_max(err):
    """max over each group's points: [n, ...] -> [3, ...] float64."""
    return np.stack([np.asarray(err[GROUP_ID == g].max(axis=0), dtype=np.float64) for g in range(3)])


@functools.lru_cache(maxsize=None)
def references(seed=0):
    """Everything the tests compare with, at degree 8 (degree d is the first
    d*d columns), computed once:

    pts        float32 [N, 3]
    val / jac  the exact values [N, 64] and Jacobian [N, 3, 64] of the table
               with its full literals (float64): the float32 kernels' target
    val32      the oracle's float32 evaluation
    val_ld / jac_ld   long-double evaluation with float32-rounded literals:
               the float64 kernels' target
    indep / indep_jac  the independent definition
    literal    [64]: how far the float32-rounded literals move a value on the
               unit group, max |val_ld - indep| (references only)
    base       {(dtype, "val"): [3, 64], (dtype, "jac"): [3, 3, 64]} for dtype
               in "f32", "f64": the references' own error per group
    """
    with np.errstate(all="ignore"):
        pts = inputs(seed)
        val = values(pts, 8, np.float64)
        val32 = values(pts, 8, np.float32)
        jac = jacobian(pts, 8, np.complex128)
        jac32 = jacobian(pts, 8, np.complex64)
        val_ld = values(pts, 8, np.longdouble, _f32_literal(np.longdouble))
        val_d = values(pts, 8, np.float64, _f32_literal(np.float64))
        jac_ld = jacobian(pts, 8, np.clongdouble, _f32_literal(np.clongdouble))
        jac_d = jacobian(pts, 8, np.complex128, _f32_literal(np.complex128))
        base = {("f32", "val"): _group_max(np.abs(val32.astype(np.float64) - val)),
                ("f32", "jac"): _group_max(np.abs(jac32.astype(np.float64) - jac)),
                ("f64", "val"): _group_max(np.abs(val_d.astype(np.longdouble) - val_ld)),
                ("f64", "jac"): _group_max(np.abs(jac_d.astype(np.longdouble) - jac_ld))}
        x, y, z = (pts[:, i].astype(np.float64) for i in range(3))
        indep = independent(x, y, z, 8)
        indep_jac = independent_jacobian(pts, 8)
        literal = np.abs(val_ld - indep.astype(np.longdouble))[GROUP_ID == 0].max(0).astype(np.float64)
    for a in (pts, val, val32, jac, val_ld, jac_ld, indep, indep_jac, literal, *base.values()):
        a.setflags(write=False)
    return types.SimpleNamespace(pts=pts, val=val, val32=val32, jac=jac, jac32=jac32, val_ld=val_ld,
                                 jac_ld=jac_ld, indep=indep, indep_jac=indep_jac, literal=literal, base=base)


def bases(seed=0):
    return references(seed).base


def band_of(column):
    return int(math.isqrt(int(column)))
