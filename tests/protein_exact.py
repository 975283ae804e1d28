"""Protein-docking energy in extended precision, and how far a correct float64 kernel may be from it.

exact_energy() restates the reference's energy (src/problem/protein_docking.py:28-48) in np.longdouble (64-bit mantissa) with the
distances taken from coordinate differences, not from the expansion |a_i|^2 - 2 a_i.a_j + |a_j|^2 that the kernels and the C oracle use.
allowance() bounds, per candidate, the distance between that value and any float64 evaluation that follows the kernels' formula.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, f'np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here: the exact protein energy needs >= 63'

U = 2.0 ** -53          # unit roundoff of float64
K = 3.5                 # roundings at the scale S_ij in the kernels' squared distance (see allowance())
PD_CUT = 9.1            # pairs beyond this distance contribute nothing, to either side (the cut-off is 9)


def tables(problem):
    """(v0, basis [D, n, 3], coor_init [n, 3], sqrt(e), q, r) from the problem's descriptor: the inputs the kernels get."""
    d = problem.desc()
    n, D = int(d['n_peaks']), int(d['dim'])
    pw = np.asarray(d['pw'], dtype=np.float64).reshape(3, n, n)
    return (np.asarray(d['v0'], dtype=np.float64), np.asarray(d['py'], dtype=np.float64).reshape(D, n, 3),
            np.asarray(d['pc'], dtype=np.float64).reshape(n, 3), pw[0], pw[1], pw[2])


def _coords(problem, X):
    v0, B, C, *_ = tables(problem)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    ev = 1 / np.sqrt(np.asarray(problem.eigval, dtype=LD)) if hasattr(problem, 'eigval') else v0.astype(LD)
    A = np.einsum('mk,kna->mna', X.astype(LD) * ev, B.astype(LD)) + C.astype(LD)
    # componentwise bound of the float64 coordinate's rounding error: a D-term dot product plus the add of coor_init
    mag = np.einsum('mk,kna->mna', np.abs(X * v0), np.abs(B))
    ea = U * ((X.shape[1] + 1) * mag + np.where(mag > 0, np.abs(C), 0.))
    return A, ea


def _pairs(A):
    """Index arrays (m, i, j) of the pairs i < j of each candidate whose distance is below PD_CUT (chosen in float64, with margin)."""
    n = A.shape[1]
    iu, ju = np.triu_indices(n, 1)
    A64 = A.astype(np.float64)
    d2 = ((A64[:, iu] - A64[:, ju]) ** 2).sum(-1) + 0.01
    m, t = np.nonzero(d2 < (PD_CUT + 0.05) ** 2)
    return m, iu[t], ju[t]


def _terms(problem, A, m, i, j):
    _, _, _, se, q, r = tables(problem)
    dv = A[m, i] - A[m, j]
    pd = np.sqrt((dv * dv).sum(-1) + LD(0.01))
    se_, q_, r_ = se[i, j].astype(LD), q[i, j].astype(LD), r[i, j].astype(LD)
    rp = r_ / pd
    r6 = rp ** 6
    r12 = r6 * r6
    coeff = q_ / (4 * pd) + se_ * (r12 - r6)
    sw = (9 - pd) ** 2 * (-12 + 2 * pd) / 8
    near = (pd > LD(0.11)) & (pd < 7)
    far = (pd > 7) & (pd < 9)
    t = np.where(near, 10 * coeff, np.where(far, 10 * coeff * sw, 0))
    return dict(pd=pd, dv=dv, coeff=coeff, sw=sw, r6=r6, r12=r12, q=q_, se=se_, t=t, near=near, far=far)


def exact_energy(problem, X):
    """Energy of every row of X [m, D] in np.longdouble: mean_j sum_i term_ij = (2 / n) sum_{i<j} term_ij (term_ii = 0: pd = 0.1)."""
    A, _ = _coords(problem, X)
    m, i, j = _pairs(A)
    tt = _terms(problem, A, m, i, j)
    out = np.zeros(A.shape[0], dtype=LD)
    np.add.at(out, m, tt['t'])
    return out * 2 / A.shape[1]


def allowance(problem, X, with_energy=False):
    """-> (allow [m] float64, n_ambiguous [m] int[, exact energy [m] longdouble]).

    A float64 kernel that follows the reference's formula computes, per pair i < j,
      s = |a_i|^2 - 2 a_i.a_j + |a_j|^2 + 0.01, pd = sqrt(s), term = 10 coeff(pd) [x sw(pd)],
    and sums the terms.  First-order error sources, u = 2^-53:
      * the expansion.  p2_i = |a_i|^2, p3 = a_i.a_j and p2_j are three-term dot products: <= 3 roundings each at the scale of
        |a_i|^2, |a_i|.|a_j| (componentwise absolute values) and |a_j|^2, i.e. <= 3 u S_ij altogether with
        S_ij = |a_i|^2 + 2 |a_i|.|a_j| + |a_j|^2; the subtraction p2_i - 2 p3 rounds at <= S_ij / 4 (a close pair has
        |p2_i - 2 p3| ~ |a|^2 ~ S_ij / 4), the two additions at s.  So |s~ - s| <= K u S'_ij with K = 3.5 (3 + 1/4, rounded up to
        cover the additions of s, which are ~1e-4 S_ij for a close pair);
      * coordinates a = sum_k x_k v0_k B_k + c: componentwise error e <= u ((D + 1) sum_k |x_k v0_k B_k| + |c|), which moves s by at
        most 2 |a_i - a_j| . (e_i + e_j): S'_ij = S_ij + 0.01 + 2 |a_i - a_j| . (e_i + e_j) / u;
      * the square root and the reciprocal: <= 2 ulp of pd.
    Together |pd~ - pd| <= E_ij = u (K S'_ij / (2 pd) + 2 pd).  The term moves by at most G_ij E_ij with G_ij = |d term / d pd| (taken in
    extended precision, switch included), and its own evaluation (~10 operations) rounds at the scale T_ij = 10 (|q| / (4 pd) +
    |sqrt(e)| (r^12 + r^6)) [x |sw|].  The sum of the <= 4950 terms -- <= 78 per lane, then a tree -- rounds by at most 86 u sum T_ij.
      allow = (2 / n) [ sum_ij (G_ij E_ij + 96 u T_ij) + sum_{ambiguous} |10 coeff_ij| ]
    At 9 the term is continuous (sw(9) = 0, sw'(9) = 0): a pair on the wrong side of 9 changes the sum by at most G_ij E_ij, which is
    covered (G is taken from the smooth continuation of the far window).  At 0.11 and 7 the term jumps (at exactly 7 it is 0, on both sides
    10 coeff): a pair whose exact pd lies within E_ij of either edge is AMBIGUOUS -- the kernel may decide either way -- and is allowed
    its jump.  The tests assert that their random candidates have none.
    """
    A, ea = _coords(problem, X)
    n = A.shape[1]
    m, i, j = _pairs(A)
    tt = _terms(problem, A, m, i, j)
    pd, dv = tt['pd'], tt['dv']
    A64, dv64 = A.astype(np.float64), np.abs(dv.astype(np.float64))
    S = (A64[m, i] ** 2).sum(-1) + 2 * np.abs(A64[m, i] * A64[m, j]).sum(-1) + (A64[m, j] ** 2).sum(-1) + 0.01
    S = S + 2 * (dv64 * (ea[m, i] + ea[m, j])).sum(-1) / U
    p = pd.astype(np.float64)
    E = U * (K * S / (2 * p) + 2 * p)
    q, se = np.abs(tt['q'].astype(np.float64)), np.abs(tt['se'].astype(np.float64))
    r6, r12 = tt['r6'].astype(np.float64), tt['r12'].astype(np.float64)
    cmag = q / (4 * p) + se * (r12 + r6)                       # |coeff| bound
    sw = tt['sw'].astype(np.float64)
    near_band = p < 7                                           # the far window's formula (its smooth continuation beyond 9) from 7 up
    pdl, cl = tt['pd'], tt['coeff']
    dc = -tt['q'] / (4 * pdl * pdl) + tt['se'] * (-12 * tt['r12'] + 6 * tt['r6']) / pdl
    dswl = (-2 * (9 - pdl) * (-12 + 2 * pdl) + 2 * (9 - pdl) ** 2) / 8
    G = 10 * np.abs(np.where(near_band, dc, dc * tt['sw'] + cl * dswl).astype(np.float64))
    T = 10 * np.where(near_band, cmag, cmag * np.abs(sw))
    T = np.where(pd > LD(0.11), T, 0.)                          # below 0.11 the term is 0: only the edge itself (ambiguous) can move it
    G = np.where(pd > LD(0.11), G, 0.)
    jump = 10 * np.abs(tt['coeff'].astype(np.float64)) * (1 + 1e-12)    # (+ the rounding of this float64 sum)
    amb = (np.abs(pd - LD(0.11)) <= E) | (np.abs(pd - 7) <= E)
    per = G * E + 96 * U * T + np.where(amb, jump, 0.)
    allow = np.zeros(A.shape[0])
    np.add.at(allow, m, per)
    namb = np.zeros(A.shape[0], dtype=np.int64)
    np.add.at(namb, m, amb.astype(np.int64))
    allow *= 2. / n
    if with_energy:
        e = np.zeros(A.shape[0], dtype=LD)
        np.add.at(e, m, tt['t'])
        return allow, namb, e * 2 / n
    return allow, namb


def check(problem, X, got, label=''):
    """|got - exact| / allowance for every row; raises with the worst rows when one exceeds 1.  Returns the largest ratio."""
    allow, namb, ex = allowance(problem, X, with_energy=True)
    err = np.abs(np.asarray(got, dtype=LD) - ex).astype(np.float64)
    ratio = err / allow
    bad = np.nonzero(~(ratio <= 1.))[0]
    assert bad.size == 0, (f'{label} {problem}: {bad.size} of {len(ratio)} rows outside the allowance; worst ratio {ratio.max():.3g}',
                           [(int(k), float(got[k]), float(ex[k]), float(allow[k]), int(namb[k])) for k in bad[np.argsort(-ratio[bad])][:5]])
    return float(ratio.max()) if len(ratio) else 0.
