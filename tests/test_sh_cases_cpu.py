"""The SH test cases' own references against one another (no GPU): the
oracle's table of 64 polynomials against the independent recurrence
definition, and the error bases that tests/test_gpu_sh.py multiplies by 4."""
import math

import numpy as np
import pytest

import oracle
import sh_cases as sc


@pytest.fixture(scope="module")
def ref():
    return sc.references()


def test_inputs_hold_every_edge(ref):
    p = ref.pts
    assert p.shape == (sc.N, 3) and p.dtype == np.float32 and np.isfinite(p).all()
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    u, h, d = (sc.GROUP_ID == g for g in range(3))
    assert np.abs(r[u] - 1).max() < 3e-7
    assert (p[h][0] == 0).all() and np.abs(r[h][1:] - 0.5).max() < 2e-7
    assert np.abs(r[d] - 2).max() < 5e-7
    sp = sc.special_unit()
    assert (p[:len(sp)].view(np.uint32) == sp.view(np.uint32)).all()
    for axis in range(3):
        for s in (1.0, -1.0):
            e = np.zeros(3, np.float32); e[axis] = s
            assert (sp == e).all(1).any()
    assert np.signbit(sp[sp == 0]).any() and not np.signbit(sp[sp == 0]).all()      # -0.0 and 0.0
    tiny = np.finfo(np.float32).tiny
    assert ((sp != 0) & (np.abs(sp) < tiny)).any()                                  # a denormal
    assert (np.abs(sp[:, 0]) == np.spacing(np.float32(1))).any()                    # the nudged poles
    # every batch size is a prefix that holds every group (one row cannot)
    for B in sc.BATCHES:
        rows = sc.batch_rows(B)
        assert len(rows) == B and len(set(rows.tolist())) == B
        if B >= 3:
            assert np.bincount(sc.GROUP_ID[rows], minlength=3).min() >= min(B // 3, sc.N_HALF)
    short = np.concatenate([sc.batch_rows(B) for B in (63, 64, 65)])
    assert set(range(len(sp))) <= set(short.tolist())


def test_independent_definition_agrees_with_the_oracle_table(ref):
    """Values and complex-step Jacobians within 1e-12 on the unit and the half
    group. The two forms are the same polynomials off the sphere as well; at
    radius 2 the values reach 2.3e3 and the Jacobian 9.2e3, so there the
    1e-12 is taken relative to each column's largest magnitude in the group
    (measured: 6e-16 of it)."""
    for g, name in enumerate(sc.GROUPS):
        m = sc.GROUP_ID == g
        dv = np.abs(ref.indep[m] - ref.val[m]).max(0)
        dj = np.abs(ref.indep_jac[m] - ref.jac[m]).max(0)
        sv = sj = 1.0
        if name == "double":
            sv = np.maximum(1.0, np.abs(ref.val[m]).max(0))
            sj = np.maximum(1.0, np.abs(ref.jac[m]).max(0))
        print(name, "values", float((dv / sv).max()), "jacobian", float((dj / sj).max()))
        assert (dv <= 1e-12 * sv).all(), (name, int(np.argmax(dv / sv)))
        assert (dj <= 1e-12 * sj).all(), (name, np.unravel_index(np.argmax(dj / sj), dj.shape))


def test_complex_step_is_the_analytic_jacobian(ref):
    """The complex step against derivatives written by hand for a few columns
    of different shape (a constant, the linear band, a z-only column, a
    sectoral column of band 7), so that the step itself is pinned."""
    p = ref.pts.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    J = ref.jac
    assert (J[:, :, 0] == 0).all()
    assert np.allclose(J[:, 1, 1], -0.48860251190291987, rtol=0, atol=1e-15)
    assert np.allclose(J[:, 2, 6], 2 * 0.94617469575755997 * z, rtol=1e-15, atol=0)
    k = 0.70716273252459627
    dx63 = k * (-35 * x**2 * y**4 + 21 * x**4 * y**2 - x**6 + 7 * y**6) \
        + k * x * (-70 * x * y**4 + 84 * x**3 * y**2 - 6 * x**5)
    scale = np.maximum(1.0, np.abs(dx63))
    assert (np.abs(J[:, 0, 63] - dx63) <= 1e-13 * scale).all()


def test_band_sums():
    """sum_m Y_lm^2 = (2l+1)/(4 pi) on directions normalised in float64 (the
    float32 unit group is off the sphere by 6e-8), for both forms."""
    p = sc.inputs()[sc.GROUP_ID == 0].astype(np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for vals in (sc.independent(x, y, z, 8), oracle._sh_values(x, y, z, 8, np.float64)):
        for l in range(8):
            s = (vals[:, l * l:(l + 1) ** 2] ** 2).sum(1)
            assert np.abs(s - (2 * l + 1) / (4 * math.pi)).max() <= 1e-12, l


@pytest.mark.parametrize("d", range(1, 9))
def test_degree_is_a_prefix_of_degree_8(ref, d):
    p = ref.pts
    with np.errstate(all="ignore"):
        assert np.array_equal(sc.values(p, d, np.float64), ref.val[:, :d * d])
        assert np.array_equal(sc.values(p, d, np.float32), ref.val32[:, :d * d])
        assert np.array_equal(oracle.sh_encode(p, d), ref.val32[:, :d * d])
        assert np.array_equal(sc.jacobian(p, d, np.complex128), ref.jac[:, :, :d * d])
        assert np.array_equal(sc.jacobian(p, d, np.complex64), ref.jac32[:, :, :d * d])
        assert np.array_equal(sc.independent(p[:, 0], p[:, 1], p[:, 2], d), ref.indep[:, :d * d])


def test_const_argument_rounds_only_the_literals(ref):
    """The default of `const` is T, so sh_encode is what it was (pinned by
    tests/test_oracle.py as well); with float32-rounded literals the float64
    evaluation moves by at most a few 2^-24 of the column's size."""
    p = ref.pts
    v = p.astype(np.float64)
    a = oracle._sh_values(v[:, 0], v[:, 1], v[:, 2], 8, np.float64)
    b = oracle._sh_values(v[:, 0], v[:, 1], v[:, 2], 8, np.float64, const=np.float64)
    assert np.array_equal(a, b)
    r = sc.values(p, 8, np.float64, sc._f32_literal(np.float64))
    assert not np.array_equal(r, a)
    for g in range(3):
        m = sc.GROUP_ID == g
        # a column is a sum of monomials whose cancellation on the sphere is
        # at most a few hundred (band 7), each literal off by 2^-25 relative
        assert (np.abs(r - a)[m].max(0) <= 2.0 ** -14 * np.maximum(1.0, np.abs(a[m]).max(0))).all()


def test_bases_are_zero_only_where_the_kernel_must_be_exact(ref):
    for (dtype, kind), base in ref.base.items():
        want = sc.structural_zero(dtype, kind)
        for g, name in enumerate(sc.GROUPS):
            assert np.isfinite(base[g]).all()
            assert np.array_equal(base[g] == 0, want), (dtype, kind, name, np.argwhere((base[g] == 0) != want)[:8])
    # the sizes the issue measured: float32 values 1.5e-8 in band 0 to about
    # 4e-6 in band 7 on the unit group, the Jacobian up to about 1e-5
    b = ref.base["f32", "val"][0]
    assert 1e-8 < b[0] < 2e-8 and 1e-7 < b[49:].max() < 1e-5
    assert 1e-6 < ref.base["f32", "jac"][0].max() < 3e-5
    assert ref.base["f64", "val"][0].max() < 1e-14
