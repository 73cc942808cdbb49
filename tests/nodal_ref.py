"""Reference of the nodal update and the boundary conditions -- TEST INFRASTRUCTURE ONLY.

Written from the reference's formulas (v2/HAKAI_j.jl:564 and :585-617), not from the oracle or the
kernels, as numpy_ref.py / hp_ref.py are for the element update:

  amplitude    the segment search and interpolation of :588-599
  apply_bc     :585-617, groups in order, entries in order, disp_new[dof] = v * amp
  nodal_step   :564 operation for operation in IEEE double
  nodal_exact  the same value in exact rationals, rounded once (the guard against a mistake that
               nodal_step and the oracle could share)

The rounding bound (nodal_terms, nodal_bound)
---------------------------------------------
With A = m / dt^2 (exact, dt the double that is stepped), W = 2u - u_pre and diag_C = 0 * m = +-0,
:564 is  x = 1 / (A + 0) * (f - Q + A * W + 0 * u_pre),  exactly  X = (f - Q) / A + W.
The terms with diag_C add or multiply a zero: they round nothing (they can only turn the sign of
a zero result, which the bit-for-bit comparisons with the oracle see). 2.0 * u is exact. What is
left rounds eight times:

  1  dt * dt            5  2u - u_pre  (W)
  2  m / (dt * dt)  (a) 6  a * W
  3  1 / a        (inv) 7  (f - Q) + a * W
  4  f - Q              8  inv * (...)

Each rounding is a factor (1 + e), |e| <= 2^-53. (f - Q) / A carries six of them (1, 2, 3, 4, 7,
8: roundings 1 and 2 enter through inv only, because a cancels in inv * (a * W) up to 3), W carries
five (3, 5, 6, 7, 8). The product of k such factors is within k * 2^-53 / (1 - k * 2^-53) of one,
which for k <= 6 is below 8 * 2^-53, so

  |x - X| <= 8 * 2^-53 * (|f - Q| / |A| + |W|) <= 8 * 2^-53 * S,
  S = (1 / |A|) * (|f| + |Q| + |A| * (2|u| + |u_pre|)),

the magnitude sum of the dof. COUNT = 8 is the number of roundings, not a fitted figure.

Underflow: sums and differences of doubles are exact when subnormal, dt * dt, a and inv are
required to be normal (nodal_terms asserts it), so only the products 6 and 8 can round into the
subnormal range, each with an absolute error of at most 2^-1075. The first is then multiplied by
inv: nodal_bound adds 2^-1074 * (1 / |A| + 1), which also covers inv's own relative error.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

COUNT = 8                       # roundings of :564, see above
U = Fraction(1, 2 ** 53)        # unit roundoff of double
TINY = Fraction(1, 2 ** 1074)   # smallest subnormal
MIN_NORMAL = 2.0 ** -1022


def amplitude(a_t, a_v, ct):
    """:588-599: the first segment j with a_t[j] <= ct <= a_t[j+1], the first one when none holds
    ct (so times outside the table extrapolate the FIRST segment); linear interpolation in the
    reference's operation order. A one-point table raises IndexError (the reference: BoundsError)."""
    a_t = [float(x) for x in a_t]
    a_v = [float(x) for x in a_v]
    ct = float(ct)
    ti = 0
    for j in range(len(a_t) - 1):
        if ct >= a_t[j] and ct <= a_t[j + 1]:
            ti = j
            break
    return a_v[ti] + (a_v[ti + 1] - a_v[ti]) * (ct - a_t[ti]) / (a_t[ti + 1] - a_t[ti])


def segment(a_t, ct):
    """The 0-based segment amplitude() interpolates on, and whether any segment holds ct."""
    for j in range(len(a_t) - 1):
        if ct >= a_t[j] and ct <= a_t[j + 1]:
            return j, True
    return 0, False


def apply_bc(model, ct, disp_new):
    """:585-617 in place: groups in order, entries in order, every dof of an entry set to v * amp
    (amp = 1.0 for a group without amplitude). Later writers overwrite earlier ones."""
    for g in model.bc:
        amp = 1.0 if g.amp_time is None else amplitude(g.amp_time, g.amp_value, ct)
        for dofs, v in g.entries:
            disp_new[np.asarray(dofs, np.int64) - 1] = float(v) * amp
    return disp_new


def nodal_step(diag_M, dt, u, u_pre, Q, f):
    """:564 for every dof, in double, one IEEE operation per operation of the source line:
    1.0 / (m/dt^2 + C/2.0/dt) * (f - Q + m/dt^2.0 * (2.0*u - u_pre) + C/2.0/dt * u_pre) with
    C = diag_C = 0 * m (:217-218) kept, as the kernel keeps it."""
    m, u, u_pre, Q, f = (np.asarray(x, np.float64) for x in (diag_M, u, u_pre, Q, f))
    dt = np.float64(dt)
    with np.errstate(all="ignore"):
        dC = 0.0 * m
        a = m / (dt * dt)
        c = dC / 2.0 / dt
        return 1.0 / (a + c) * (f - Q + a * (2.0 * u - u_pre) + c * u_pre)


def nodal_terms(diag_M, dt, u, u_pre, Q, f):
    """Per dof, in exact rationals: X, the value of :564 without any rounding, S, the magnitude sum
    the rounding bound is relative to, and 1 / |A|. Asserts the operands are in scope: finite,
    nonzero mass, dt * dt, m / dt^2 and its reciprocal normal."""
    m, u, u_pre, Q, f = (np.asarray(x, np.float64) for x in (diag_M, u, u_pre, Q, f))
    dtf = Fraction(float(dt))
    assert abs(float(dt) * float(dt)) >= MIN_NORMAL
    X, S, inv_A = [], [], []
    for i in range(m.shape[0]):
        assert np.isfinite([m[i], u[i], u_pre[i], Q[i], f[i]]).all() and m[i] != 0.0
        A = Fraction(float(m[i])) / (dtf * dtf)
        assert MIN_NORMAL * 4 <= abs(A) <= 2.0 ** 1020, "m / dt^2 or its reciprocal out of the normal range"
        ui, pi, qi, fi = (Fraction(float(x[i])) for x in (u, u_pre, Q, f))
        X.append((fi - qi) / A + (2 * ui - pi))
        S.append((abs(fi) + abs(qi)) / abs(A) + 2 * abs(ui) + abs(pi))
        inv_A.append(1 / abs(A))
    return X, S, inv_A


def nodal_exact(diag_M, dt, u, u_pre, Q, f):
    """:564 in exact rationals, rounded to double once (float(Fraction) rounds to nearest even)."""
    X, _, _ = nodal_terms(diag_M, dt, u, u_pre, Q, f)
    return np.array([float(x) for x in X])


def nodal_bound(S, inv_A):
    """|nodal_step - X| <= this, per dof (exact rationals): COUNT roundings of 2^-53 relative to S,
    plus the two products that may underflow (module docstring)."""
    return [COUNT * U * s + TINY * (ia + 1) for s, ia in zip(S, inv_A)]
