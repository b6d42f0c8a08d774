"""Coefficient vectors of the usual two-species reactions for ReactionDiffusion.set_state (include/smg.h: smg_rd_set_state).

A reaction is a pair of bivariate cubics (R_u, R_v) in (u, v): 20 doubles, R_u's ten coefficients first, each over the monomials of MONOMIALS in
that order.  These functions are data, not kernel variants: the one kernel k_rd_react evaluates whichever table a column is given."""
import numpy as np

MONOMIALS = ("1", "u", "v", "uu", "uv", "vv", "uuu", "uuv", "uvv", "vvv")
_IDX = {name: i for i, name in enumerate(MONOMIALS)}


def cubic(Ru=None, Rv=None):
    """the 20-vector of R_u = sum Ru[name] monomial and R_v likewise; Ru, Rv: dicts over MONOMIALS"""
    c = np.zeros(20)
    for off, terms in ((0, Ru or {}), (10, Rv or {})):
        for name, val in terms.items():
            c[off + _IDX[name]] = float(val)
    return c


def evaluate(coeff, u, v):
    """(R_u, R_v) of a 20-vector at (u, v), in the kernel's operation order (csrc/smg_rd_inl.hpp: rd_cubic)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    uu, uv, vv = u * u, u * v, v * v
    out = []
    for c in (coeff[:10], coeff[10:]):
        r = c[0] + 0.0 * u
        r = r + c[1] * u
        r = r + c[2] * v
        r = r + c[3] * uu
        r = r + c[4] * uv
        r = r + c[5] * vv
        r = r + c[6] * (uu * u)
        r = r + c[7] * (uu * v)
        r = r + c[8] * (u * vv)
        r = r + c[9] * (vv * v)
        out.append(r)
    return out[0], out[1]


def gray_scott(F, kappa):
    """R_u = -u v^2 + F (1 - u),  R_v = u v^2 - (F + kappa) v   (u the substrate, v the activator; feed F, kill kappa)"""
    return cubic(dict([("1", F), ("u", -F), ("uvv", -1.0)]), dict(uvv=1.0, v=-(F + kappa)))


def fitzhugh_nagumo(a, b, eps):
    """R_u = u - u^3 / 3 - v,  R_v = eps (u + a - b v)"""
    return cubic(dict(u=1.0, uuu=-1.0 / 3.0, v=-1.0), dict([("1", eps * a), ("u", eps), ("v", -(eps * b))]))


def schnakenberg(a, b, gamma):
    """R_u = gamma (a - u + u^2 v),  R_v = gamma (b - u^2 v)"""
    return cubic(dict([("1", gamma * a), ("u", -gamma), ("uuv", gamma)]), dict([("1", gamma * b), ("uuv", -gamma)]))


def brusselator(a, b):
    """R_u = a - (b + 1) u + u^2 v,  R_v = b u - u^2 v"""
    return cubic(dict([("1", a), ("u", -(b + 1.0)), ("uuv", 1.0)]), dict(u=b, uuv=-1.0))


def allen_cahn(eps):
    """R_u = (u - u^3) / eps^2,  R_v = 0   (one species; v is diffused alone)"""
    s = 1.0 / (eps * eps)
    return cubic(dict(u=s, uuu=-s))


def fisher_kpp(r):
    """R_u = r u (1 - u),  R_v = 0   (one species; v is diffused alone)"""
    return cubic(dict(u=r, uu=-r))


def linear(J):
    """R_u = J[0][0] u + J[0][1] v,  R_v = J[1][0] u + J[1][1] v"""
    J = np.asarray(J, dtype=np.float64).reshape(2, 2)
    return cubic(dict(u=J[0, 0], v=J[0, 1]), dict(u=J[1, 0], v=J[1, 1]))
