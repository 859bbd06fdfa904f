"""References and seeded row builders for the consumers of the neighbour lists: the NVT / CPSD votes, the tensor sums,
the eigen-decompositions, VU smoothing, classification and the five position steps (numpy; the float32 eigen-solver
and the float32 steps are oracle/pcd_oracle.py's).

* vote_judge / normal_vote_judge   float64 judges of the binary votes: forced in, forced out, or undecided where a
                                   float32 evaluation may legitimately land on either side.
* tensor_f32 / cov_f32             the voters' sums in list order, every product and add rounded to float32.
* admissible_decompositions        every eigen-decomposition a row may have given its undecided pairs (2^u candidates).
* step_f64                         the position steps in float64 (sizes the flat / new allowance only).
* the builders                     threshold_rows, scale_rows, fallback_rows, odd_normal_rows, normal_rows, eigen_cases,
                                   vu_cases, class_cases, step_cases: the rows on which a kernel's comparison direction,
                                   fallback, clamp or tie order shows.
"""
import itertools
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24                          # unit roundoff of float32
EPS_NORMALIZE = float(F32(1e-12))       # F.normalize's eps as a float32 tensor op clamps with it
FORCED_OUT, FORCED_IN, UNDECIDED = 0, 1, 2
MAX_U = 4                               # rows with more undecided pairs are not judged (2^u candidates)
RHOS = (5 * math.pi / 12, math.pi / 3, 0.3)
SPECIAL_RHOS = (0.0, math.pi / 2, math.pi / 2 + 0.01, -1.0)
T6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def _rng(name):
    return np.random.default_rng([int(b) for b in name.encode()])


def segments(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _pow2(x):
    """x is +-2^e, a normal float32: a division by it and a product with it are exact."""
    x = np.abs(x.astype(np.float64))
    m, _ = np.frexp(x)
    return (m == 0.5) & (x >= 2.0 ** -126)


def _angle_band(c_lo, c_hi, rho):
    """The votes of acosf(c) > rho / <= rho for every c in [c_lo, c_hi] (float64, inside [-1, 1]) and every acosf
    within 2 ulps of acos: (lowest, highest) float64 angle the float32 code may compare with float32(rho)."""
    with np.errstate(invalid="ignore"):
        th_lo = np.arccos(np.clip(c_hi, -1.0, 1.0))
        th_hi = np.arccos(np.clip(c_lo, -1.0, 1.0))
    e_lo = np.where(th_lo > 0, 2.0 * np.spacing(th_lo.astype(F32)).astype(np.float64), 0.0)
    e_hi = np.where(th_hi > 0, 2.0 * np.spacing(th_hi.astype(F32)).astype(np.float64), 0.0)
    return th_lo - e_lo, th_hi + e_hi


def vote_judge(pos, n, ci, off, nbr, rho):
    """The better-filtered NVT vote  acos(|clip(normalize(v_j - v_i) . n_j, -1, 1)|) > rho  judged in float64.

    dv = v_j - v_i is ONE float32 subtraction per component (the kernels and the reference both take it so); from
    there on float64: den = max(||dv||, eps) with eps = float32(1e-12) (F.normalize), c64 = |clip(dv . n_j / den)|,
    rho = float64(float32(rho)).  Returns int8 per pair: FORCED_IN (votes), FORCED_OUT, UNDECIDED.

    Which float32 results are admissible.  A float32 evaluation computes ||dv|| (three squares, two adds, a square
    root: relative error <= 2.5u, u = 2^-24), three quotients (+u each -> 3.5u per component), three products (+u ->
    4.5u) and two adds (<= 2u of the partial sums, each at most S = sum_k |dn_k n_jk|), so

        |c32 - c64| <= gamma_n = 7u S,    S <= ||n_j||_1   since |dn_k| <= 1

    (below the F.normalize eps the clamp, not the norm, is the divisor, and the bound holds a fortiori).  Then acosf
    is within 2 ulps of acos (one ulp asked of the libraries, one spare), so the code compares an angle in
    [acos(c64 + gamma_n) - e, acos(c64 - gamma_n) + e], e = 2 ulp32 of that angle, with rho.  A pair is FORCED_IN when the
    whole interval is > rho, FORCED_OUT when none of it is, UNDECIDED otherwise.  In c this is |c64 - cos(rho)| <=
    gamma_n + e sin(rho) <= 7u ||n_j||_1 + 4u: TIGHTER than the 8u (1 + ||n_j||_1) of a first-order bound (and far
    inside 2^-20 (1 + ||n_j||_1)), and exact where the first-order map of an angle error into c breaks down (rho = 0).
    Two cases are tighter still:
      * dv has one non-zero component, it is a power of two and not below the F.normalize eps (where the divisor is
        float32(1e-12) and the quotient rounds): the norm, the quotients (+-1, 0) and the dot are
        exact, c32 = c64 = |n_jk|, gamma_n = 0 -- only acosf's 2 ulps remain (threshold_rows' axis rows);
      * acos(1) = 0 is exact in every libm (e = 0 at c = 1).
    A coincident pair (dv == 0) has c = 0: decided by acos(0) > rho alone (float32(pi/2) > float32(rho)), the constant
    the kernels use.  A NaN c (NaN or inf normal, NaN position) never votes for rho >= 0 whether the clip propagates
    the NaN (torch.clamp) or drops it (fmaxf); for rho < 0 the two clips differ, so the pair is UNDECIDED."""
    pos, n = _f32(pos), _f32(n)
    seg = segments(off)
    rho64 = float(F32(rho))
    with np.errstate(all="ignore"):
        dv = (pos[nbr] - pos[np.asarray(ci)[seg]]).astype(F32)          # the one float32 subtraction
        d = dv.astype(np.float64)
        nj = n[nbr].astype(np.float64)
        den = np.maximum(np.sqrt((d * d).sum(1)), EPS_NORMALIZE)
        dn = d / den[:, None]
        terms = dn * nj
        raw = np.abs(terms.sum(1))
        c = np.minimum(raw, 1.0)
        exact = ((dv != 0).sum(1) == 1) & _pow2(np.abs(dv).max(1)) & np.isfinite(nj).all(1) \
            & (np.abs(d).max(1) >= EPS_NORMALIZE)        # (below the eps the divisor is float32(1e-12), no power of two)
        gam = np.where(exact, 0.0, 7.0 * U * np.abs(terms).sum(1))          # (before the clip, which only narrows it)
        lo, hi = _angle_band(np.clip(raw - gam, 0.0, 1.0), np.minimum(raw + gam, 1.0), rho64)
        out = np.full(len(seg), UNDECIDED, np.int8)
        out[lo > rho64] = FORCED_IN
        out[hi <= rho64] = FORCED_OUT
        zero = (dv == 0).all(1)
        out[zero] = FORCED_IN if float(F32(math.pi / 2)) > rho64 else FORCED_OUT
        nan = np.isnan(c) & ~zero
        out[nan] = FORCED_OUT if rho64 >= 0 else UNDECIDED
    return out


def pair_c64(pos, n, ci, off, nbr):
    """|clip(normalize(v_j - v_i) . n_j)| per pair in float64, as vote_judge takes it (NaN where it is not a number)."""
    pos, n = _f32(pos), _f32(n)
    with np.errstate(all="ignore"):
        d = (pos[nbr] - pos[np.asarray(ci)[segments(off)]]).astype(F32).astype(np.float64)
        den = np.maximum(np.sqrt((d * d).sum(1)), EPS_NORMALIZE)
        return np.minimum(np.abs((d / den[:, None] * n[nbr].astype(np.float64)).sum(1)), 1.0)


def normal_vote_judge(n, ci, off, nbr, rho):
    """CPSD's vote  acos(clip(n_i . n_j, -1, 1)) <= rho  (no abs, <=) judged the same way: c64 the float64 dot of the
    float32 normals, |c32 - c64| <= gamma_n = 3u sum_k |n_ik n_jk| (three products, two adds), 0 where n_i is +-e_k (the
    products with 0 and +-1 are exact), then acosf within 2 ulps.  FORCED_IN: every admissible angle <= rho."""
    n = _f32(n)
    seg = segments(off)
    rho64 = float(F32(rho))
    with np.errstate(all="ignore"):
        ni = n[np.asarray(ci)[seg]].astype(np.float64)
        nj = n[nbr].astype(np.float64)
        terms = ni * nj
        c = np.clip(terms.sum(1), -1.0, 1.0)
        exact = ((ni != 0).sum(1) == 1) & (np.abs(ni).max(1) == 1.0) & np.isfinite(nj).all(1)
        gam = np.where(exact, 0.0, 3.0 * U * np.abs(terms).sum(1))
        lo, hi = _angle_band(np.maximum(c - gam, -1.0), np.minimum(c + gam, 1.0), rho64)
        out = np.full(len(seg), UNDECIDED, np.int8)
        out[hi <= rho64] = FORCED_IN
        out[lo > rho64] = FORCED_OUT
        out[np.isnan(c)] = FORCED_OUT
    return out


def _list_order_sums(vals, off, votes):
    """sum over the voting members of vals [E, q] per row, in list order, every add rounded to float32 -> [m, q]."""
    m = len(off) - 1
    lens = np.diff(off)
    acc = np.zeros((m, vals.shape[1]), F32)
    with np.errstate(all="ignore"):
        for t in range(int(lens.max()) if m else 0):
            rows = np.nonzero(lens > t)[0]
            e = off[rows] + t
            v = votes[e]
            acc[rows[v]] = (acc[rows[v]] + vals[e[v]]).astype(F32)
    return acc


def tensor_f32(n, rows, votes):
    """T_i = sum_j w n_j n_j^T / sum w of getBetterFilteredNVT as a sequential float32 program: the six products
    (w n_jx) n_jy of every member added in list order (product and add each rounded to float32), divided by
    float32(sum w); a row with no voter is summed over every member (all weights := 1).  rows = (off, nbr); votes bool
    per pair.  -> (t6 [m, 6] in the order a00 a01 a02 a11 a12 a22, wsum int64 [m]).  For finite normals this is the sum
    over the voters; a non-voting member still enters as 0 * n_j n_j^T, as in the reference's w[..., None, None] * outer,
    so a NaN or infinite normal poisons every row that lists it, voting or not."""
    off, nbr = rows
    n = _f32(n)
    votes = np.asarray(votes, bool).copy()
    seg = segments(off)
    wsum = np.bincount(seg[votes], minlength=len(off) - 1)
    votes[(wsum == 0)[seg]] = True
    wsum = np.bincount(seg, weights=votes, minlength=len(off) - 1).astype(np.int64)
    nj = n[nbr]
    with np.errstate(all="ignore"):
        nw = np.where(votes[:, None], nj, F32(0))
        prod = np.stack([nw[:, a] * nj[:, b] for a, b in T6], 1).astype(F32)
        acc = _list_order_sums(prod, off, np.ones(len(nbr), bool))
        return (acc / wsum.astype(F32)[:, None]).astype(F32), wsum


def normal_tensor_f32(n, ci, rows, votes):
    """getNormalFilteredNVT's tensor the same way; a row where nobody votes (an empty one included) is n_i n_i^T."""
    off, nbr = rows
    n = _f32(n)
    votes = np.asarray(votes, bool)
    wsum = np.bincount(segments(off)[votes], minlength=len(off) - 1).astype(np.int64)
    nj = n[nbr]
    with np.errstate(all="ignore"):
        prod = np.stack([nj[:, a] * nj[:, b] for a, b in T6], 1).astype(F32)
        t6 = (_list_order_sums(prod, off, votes) / wsum.astype(F32)[:, None]).astype(F32)
        ni = n[np.asarray(ci)]
        none = wsum == 0
        t6[none] = np.stack([ni[none, a] * ni[none, b] for a, b in T6], 1)
    return t6, wsum


def cov_f32(pos, n, ci, rows, votes):
    """getNormalFilteredPVT's covariance: the voters' centroid (list-order float32 sums over float32(sum w)), then
    sum (v_j - c)(v_j - c)^T over the voters in list order over float32(sum w); nobody votes: everybody does; an
    empty row: the four samples +-(n x v), +-(n x (n x v))."""
    off, nbr = rows
    pos, n = _f32(pos), _f32(n)
    votes = np.asarray(votes, bool).copy()
    seg = segments(off)
    m = len(off) - 1
    votes[(np.bincount(seg[votes], minlength=m) == 0)[seg]] = True
    wsum = np.bincount(seg, weights=votes, minlength=m).astype(np.int64)
    with np.errstate(all="ignore"):
        c = F32(1) * wsum.astype(F32)
        ctr = (_list_order_sums(pos[nbr], off, votes) / c[:, None]).astype(F32)
        dv = (pos[nbr] - ctr[seg]).astype(F32)
        prod = np.stack([dv[:, b] * dv[:, a] for a, b in T6], 1).astype(F32)
        t6 = (_list_order_sums(prod, off, votes) / c[:, None]).astype(F32)
        empty = np.nonzero(np.diff(off) == 0)[0]
        if len(empty):
            en, ev = n[np.asarray(ci)[empty]], pos[np.asarray(ci)[empty]]
            s1 = np.cross(en, ev).astype(F32)
            s2 = np.cross(en, s1).astype(F32)
            acc = np.zeros((len(empty), 6), F32)
            for s in (s1, -s1, s2, -s2):
                acc = (acc + np.stack([s[:, b] * s[:, a] for a, b in T6], 1).astype(F32)).astype(F32)
            t6[empty] = acc
    return t6, wsum


def full3(t6):
    t6 = np.asarray(t6)
    T = np.empty((len(t6), 3, 3), t6.dtype)
    for q, (a, b) in enumerate(T6):
        T[:, a, b] = T[:, b, a] = t6[:, q]
    return T


def admissible_decompositions(n, rows, state, kind="nvt", pos=None, ci=None):
    """Every decomposition the rows may have: a row with u undecided pairs has 2^u vote patterns (u <= MAX_U), each
    with its tensor (kind "nvt": tensor_f32; "normal": normal_tensor_f32; "pvt": cov_f32, which take pos / ci) and
    oracle.pcd_oracle.eigh of it; u = 0 gives the one.  Returns a dict: row [c] the row of candidate c, combo [c] its
    pattern number (bit b = the vote of the row's b-th undecided pair), eigval [c, 3], eigvec [c, 3, 3], t6 [c, 6],
    wsum [c]; u [m] the undecided pairs per row; unjudged: the rows with u > MAX_U (they get no candidate)."""
    from oracle import pcd_oracle as O
    off, nbr = rows
    off = np.asarray(off, np.int64)
    nbr = np.asarray(nbr, np.int64)
    state = np.asarray(state)
    seg = segments(off)
    m = len(off) - 1
    u = np.bincount(seg[state == UNDECIDED], minlength=m)
    judged = u <= MAX_U
    # the candidates as a CSR of their own: row r repeated once per pattern, each copy with its votes
    c_row, c_combo, c_nbr, c_votes = [], [], [], []
    for r in np.nonzero(judged)[0]:
        sl = slice(off[r], off[r + 1])
        base = state[sl] == FORCED_IN
        und = np.nonzero(state[sl] == UNDECIDED)[0]
        for combo in range(1 << len(und)):
            v = base.copy()
            v[und] = [(combo >> b) & 1 for b in range(len(und))]
            c_row.append(r); c_combo.append(combo); c_nbr.append(nbr[sl]); c_votes.append(v)
    row = np.asarray(c_row, np.int64)
    c_off = _csr([len(x) for x in c_nbr])
    c_nbr = np.concatenate(c_nbr) if c_nbr else np.zeros(0, np.int64)
    c_votes = np.concatenate(c_votes) if c_votes else np.zeros(0, bool)
    if kind == "nvt":
        t6, wsum = tensor_f32(n, (c_off, c_nbr), c_votes)
    elif kind == "normal":
        t6, wsum = normal_tensor_f32(n, np.asarray(ci)[row], (c_off, c_nbr), c_votes)
    else:
        t6, wsum = cov_f32(pos, n, np.asarray(ci)[row], (c_off, c_nbr), c_votes)
    w, v = O.eigh(full3(t6))
    return dict(row=row, combo=np.asarray(c_combo, np.int64), eigval=w, eigvec=v, t6=t6, wsum=wsum, u=u,
                unjudged=np.nonzero(~judged)[0])


def same_bits(a, b):
    """Elementwise: the same float32 bits, or NaN in both (a NaN's payload and sign are not part of the contract)."""
    a, b = _f32(a), _f32(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def match_candidates(cands, m, *pairs):
    """pairs: (device [m, ...], field name of cands).  -> (ok bool [m], taken int64 [m]): row r is bit-equal (NaN
    pattern included) in every pair to one of its candidates; taken = that candidate's combo (-1: none).  Unjudged
    rows are ok = False, taken = -2."""
    ok = np.zeros(m, bool)
    taken = np.full(m, -1, np.int64)
    taken[cands["unjudged"]] = -2
    hit = np.ones(len(cands["row"]), bool)
    for dev, name in pairs:
        dev = np.asarray(dev)
        hit &= same_bits(dev[cands["row"]], cands[name]).reshape(len(hit), -1).all(1)
    for c in np.nonzero(hit)[0][::-1]:
        ok[cands["row"][c]] = True
        taken[cands["row"][c]] = cands["combo"][c]
    return ok, taken


# --------------------------------------------------------------------------------------------------- vote builders
def _csr(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off


def _unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perp(rng, u):
    p = rng.standard_normal(u.shape)
    p -= (p * u).sum(-1, keepdims=True) * u
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def _at_cos(u, p, a, length):
    """Normals of the given length whose component along the unit direction u is a (so c = a whatever the length)."""
    b = np.sqrt(np.maximum(length * length - a * a, 0.0))
    return a[..., None] * u + b[..., None] * p


def _assemble(dv, nj, lens=None):
    """Point 0 = the centre of every row at the origin with a zero normal; the pairs after it, row after row."""
    dv = np.asarray(dv, np.float64).reshape(-1, 3)
    nj = np.asarray(nj, np.float64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        pos = np.concatenate([np.zeros((1, 3), F32), dv.astype(F32)])
        n = np.concatenate([np.zeros((1, 3), F32), nj.astype(F32)])
    off = _csr(lens)
    return pos, n, np.zeros(len(lens), np.int64), off, 1 + np.arange(len(dv), dtype=np.int64)


def threshold_value(rho):
    """The |c| at which the vote flips, as a float32 in [0, 1]: cos(float32(rho)), 0 for rho >= pi/2 (no |c| votes),
    1 for rho <= 0."""
    r = float(F32(rho))
    return F32(min(max(math.cos(r), 0.0), 1.0)) if 0 <= r else F32(1.0)


def threshold_rows(rho, unit=True, k=32):
    """Rows 0-7: dv along an axis at a power-of-two length (normalisation exact, c = |n_jk| exactly), |n_jk| at the 256
    float32 neighbours of the threshold (neighbour t*8 + r - 128 in row r, slot t: consecutive neighbours go to
    different rows so that no row holds more than MAX_U undecided pairs), both signs; a threshold of 0 (rho >= pi/2)
    takes the multiples of 2^-26 instead of the subnormal neighbours of 0, values past 1 stay 1 (the clip).
    Rows 8-263: random pairs, three per row with |c| = cos(rho) (1 + rel), rel in +-{1e-8, 1e-7, 1e-6} or 0 (most of
    them undecided), the rest with rel in +-{1e-5 .. 1e-2} (decided, on the squared test's margin) or random normals.
    Normal lengths in [0.9, 1.1] (unit) or [0.25, 4]; |dv| in 1e-4 .. 1e2."""
    rng = _rng(f"threshold{float(F32(rho)):.6f}{unit}")
    ct = threshold_value(rho)
    m = 8 + 256
    u = _unit(rng, (m, k))
    p = _perp(rng, u)
    near = np.array([-1e-6, -1e-7, -1e-8, 0.0, 1e-8, 1e-7, 1e-6])
    far = np.array([s * 10.0 ** e for s in (-1, 1) for e in (-5, -4, -3, -2)])
    rel = rng.choice(far, size=(m, k))
    slots = np.argsort(rng.random((m, k)), axis=1)[:, :3]
    np.put_along_axis(rel, slots, rng.choice(near, size=(m, 3)), axis=1)
    if float(ct) == 1.0:
        rel = -np.abs(rel)                      # |c| cannot pass 1: the decided pairs sit below it
    a = np.clip(float(ct) * (1 + rel), 0.0, 1.0)
    if float(ct) == 0.0:
        a = np.abs(rel)
    a = a * rng.choice([-1.0, 1.0], size=(m, k))
    length = rng.uniform(0.9, 1.1, (m, k)) if unit else 2.0 ** rng.uniform(-2, 2, (m, k))
    nj = _at_cos(u, p, a, np.maximum(length, np.abs(a)))
    rnd = rng.random((m, k)) < 0.2
    np.put_along_axis(rnd, slots, False, axis=1)
    nj[rnd] = rng.standard_normal((int(rnd.sum()), 3)) * length[rnd][:, None]
    dv = u * (10.0 ** rng.uniform(-4, 2, (m, k)))[..., None]
    for r in range(8):
        i = np.arange(k) * 8 + r - 128
        if float(ct) == 0.0:
            sel = ((i + 128) * 2.0 ** -26).astype(F32)
        else:
            sel = (ct.astype(np.float64) + i * float(np.spacing(ct))).astype(F32) if float(ct) < 1.0 else \
                (1.0 + i * 2.0 ** -24).astype(F32)
        axis = r % 3
        dv[r] = 0
        dv[r, :, axis] = 2.0 ** (r - 3) * (1 if r % 2 == 0 else -1)
        nj[r] = 0
        nj[r, :, axis] = sel.astype(np.float64) * (1 if r < 4 else -1)
        nj[r, :, (axis + 1) % 3] = np.sqrt(np.maximum(1 - sel.astype(np.float64) ** 2, 0))
    return _assemble(dv, nj, [k] * m)


SCALE_LENGTHS = (2.0 ** -70, 2.0 ** -45, 1e-13, 1e-12, 2.0 ** -39, 1.0, 2.0 ** 52, 2.0 ** 60)


def scale_rows(rho, k0=16):
    """|dv| in SCALE_LENGTHS: |dv|^2 subnormal or 0 in float32, below the kernels' 1e-24 guard, below, at and just above
    the F.normalize eps (where the clamp changes c), ordinary, and past the 1e30 guard without overflow.  Per length
    one row along an axis and three in random directions; c well away from the threshold except ONE pair per row
    within 1e-6 of it (returned as near [E] bool: the only pairs that may be undecided)."""
    rng = _rng(f"scale{float(F32(rho)):.6f}")
    ct = float(threshold_value(rho))
    dvs, njs, nears = [], [], []
    lens = []
    for L in SCALE_LENGTHS:
        for var in range(4):
            k = 4 if L < 1e-20 else k0      # (the clamped c ~ 1e-10 of these is undecided at rho = pi/2: <= MAX_U a row)
            lens.append(k)
            u = _unit(rng, (k,))
            if var == 0:
                u = np.zeros((k, 3)); u[:, rng.integers(0, 3)] = rng.choice([-1.0, 1.0], k)
            p = _perp(rng, u + 1e-3 * _unit(rng, (k,))) if var == 0 else _perp(rng, u)
            p -= (p * u).sum(-1, keepdims=True) * u
            p /= np.linalg.norm(p, axis=-1, keepdims=True)
            # the clamp den = max(|dv|, eps) scales c by |dv| / eps below the eps: aim the NORMAL's component so that
            # the clamped c sits where intended
            shrink = min(L / EPS_NORMALIZE, 1.0)
            c = np.clip(ct + rng.choice([-0.3, -0.1, 0.1, 0.3], k) * (1.0 if 0.35 < ct < 0.65 else 0.5), 0.02, 0.98)
            near = np.zeros(k, bool)
            if shrink > 0.05:
                near[rng.integers(0, k)] = True
                c[near] = np.clip(ct + rng.choice([-1.0, 1.0]) * rng.uniform(0, 1e-6), 0.0, 1.0)
            a = c / shrink if shrink > 0.05 else rng.uniform(0.1, 0.9, k)
            a = a * rng.choice([-1.0, 1.0], k)
            nj = _at_cos(u, p, a, np.maximum(1.0, np.abs(a)))
            dvs.append(u * L); njs.append(nj); nears.append(near)
    return _assemble(np.concatenate(dvs), np.concatenate(njs), lens) + (np.concatenate(nears),)


FALLBACK_LENGTHS = (1, 2, 31, 32, 33, 64, 65, 200)


def fallback_rows(exact=False):
    """Per length in FALLBACK_LENGTHS three rows: nobody votes (every normal parallel to its dv: the all-ones
    fallback), only the LAST member votes, and every member is a copy of the centre (dv == 0, the constant vote) --
    with an empty row in the middle of the CSR and one at its end.  Normals random, lengths in [0.9, 1.1].
    exact: dv and its normal along one axis, |dv| a power of two and |n_j| in [1, 1.1], so c is exactly 1 after the clip
    (and exactly 0 for the perpendicular voter): the rows for rho = 0, where a c of 1 - 1e-7 votes."""
    rng = _rng("fallback")
    dvs, njs, lens = [], [], []
    for k in FALLBACK_LENGTHS:
        for var in range(3):
            u = _unit(rng, (k,))
            s = rng.uniform(0.9, 1.1, (k, 1)) * rng.choice([-1.0, 1.0], (k, 1))
            nj = u * s                                                # parallel: c = 1, no vote for any rho >= 0
            dv = u * (10.0 ** rng.uniform(-3, 1, (k, 1)))
            if exact:
                ax = rng.integers(0, 3, k)
                u = np.eye(3)[ax]
                nj = u * (1.0 + np.abs(s) - 0.9) * np.sign(s)
                dv = u * 2.0 ** rng.integers(-8, 4, (k, 1)) * rng.choice([-1.0, 1.0], (k, 1))
            if var == 1:
                nj[-1] = (np.eye(3)[(ax[-1] + 1) % 3] if exact else _perp(rng, u[-1:])[0]) * s[-1]   # c = 0: votes below pi/2
            if var == 2:
                dv[:] = 0.0
                nj = rng.standard_normal((k, 3))
            dvs.append(dv); njs.append(nj); lens.append(k)
        if k == 32:
            lens.append(0)
    lens.append(0)
    return _assemble(np.concatenate(dvs), np.concatenate(njs), lens)


def odd_normal_rows(k=12):
    """A zero normal, a NaN normal and normals of length 1e-20 and 1e15, each a member of two rows of otherwise ordinary
    pairs (one row where other members vote at 5pi/12, one where the odd member sits among non-voters)."""
    rng = _rng("odd_normals")
    odd = [np.zeros(3), np.full(3, np.nan), _unit(rng, ())* 1e-20, _unit(rng, ()) * 1e15]
    dvs, njs = [], []
    for o in odd:
        for var in range(2):
            u = _unit(rng, (k,))
            p = _perp(rng, u)
            a = rng.uniform(0.02, 0.15, k) if var == 0 else rng.uniform(0.97, 0.995, k)
            nj = _at_cos(u, p, a * rng.choice([-1.0, 1.0], k), np.ones(k))
            nj[k // 2] = o
            dvs.append(u * (10.0 ** rng.uniform(-2, 0, (k, 1)))); njs.append(nj)
    return _assemble(np.stack(dvs), np.stack(njs), [k] * len(dvs))


NORMAL_RHOS = (0.9, 0.3)


def normal_rows(rho):
    """CPSD rows: the centre (point 0) has n_i = e_x, a member's n_j = (a, sqrt(1 - a^2) (cos t, sin t)) so n_i . n_j
    = a exactly.  Rows of 65, 100 and 200 members (and 8, 64): voters only among the members 64 and later, only among
    0-63, everywhere, nowhere; two members per row at the float32 neighbours of cos(rho) (-2 .. +2 ulps across the
    rows); an empty row in the middle and at the end.  Positions: dyadic, random."""
    rng = _rng(f"normal{rho}")
    ct = F32(math.cos(float(F32(rho))))
    pos, n, lens = [np.zeros((1, 3))], [np.array([[1.0, 0.0, 0.0]])], []
    row = 0
    for k in (8, 64, 65, 100, 200):
        for var in ("late", "early", "all", "none"):
            if var == "late" and k <= 64:
                continue
            a_in = rng.uniform(float(ct) + 0.02, 1.0, k)
            a_out = rng.uniform(-1.0, float(ct) - 0.02, k)
            t = np.arange(k)
            voter = {"late": t >= 64, "early": t < min(64, k - 1) if k > 64 else t < k // 2, "all": t >= 0,
                     "none": t < 0}[var]
            a = np.where(voter, a_in, a_out).astype(F32).astype(np.float64)
            if var != "none":
                for s, slot in enumerate(((k - 1, k - 3) if var == "late" else (1, 5)) if k >= 8 and not
                                         (var == "late" and k < 67) else ()):
                    a[slot] = float(ct) + ((row + 3 * s) % 5 - 2) * float(np.spacing(ct))
            ang = rng.uniform(0, 2 * math.pi, k)
            b = np.sqrt(np.maximum(1 - a * a, 0))
            n.append(np.stack([a, b * np.cos(ang), b * np.sin(ang)], 1))
            pos.append(rng.integers(-64, 65, (k, 3)) / 64.0)
            lens.append(k); row += 1
        if k == 65:
            lens.append(0); row += 1
    lens.append(0)
    pos, n = _f32(np.concatenate(pos)), _f32(np.concatenate(n))
    off = _csr(lens)
    return pos, n, np.zeros(len(lens), np.int64), off, 1 + np.arange(off[-1], dtype=np.int64)


# ------------------------------------------------------------------------------------------- eigen / VU / classes
def _t6_of(T):
    T = np.asarray(T)
    return np.stack([T[..., a, b] for a, b in T6], -1)


def eigen_cases():
    """(names, t6 float32 [m, 6]): zero, identity/3, diagonals with two and three equal entries, rank 1 and 2 along
    the axes and along (1,1,1), entries at float32(0.3), the scales 2^-140, 2^-100, 2^60, one NaN entry, one inf entry
    and 512 random PSD tensors (the last block)."""
    rng = _rng("eigen")
    cases = []
    add = lambda name, T: cases.append((name, np.asarray(T, np.float64)))
    add("zero", np.zeros((3, 3)))
    add("identity/3", np.eye(3) / 3)
    add("diag_aab", np.diag([0.25, 0.25, 0.5]))
    add("diag_abb", np.diag([0.25, 0.5, 0.5]))
    add("diag_aba", np.diag([0.5, 0.25, 0.5]))
    add("diag_aaa", np.diag([0.75, 0.75, 0.75]))
    for ax in range(3):
        e = np.eye(3)[ax]
        add(f"rank1_e{ax}", np.outer(e, e))
        add(f"rank2_e{ax}", np.eye(3) - np.outer(e, e))
    one = np.ones(3)
    add("rank1_111", np.outer(one, one) / 3)
    add("rank1_111_unnormalised", np.outer(one, one))
    add("rank2_111", np.eye(3) - np.outer(one, one) / 3)
    add("rank2_111_110", np.outer(one, one) + np.outer([1, -1, 0], [1, -1, 0]))
    t = float(F32(0.3))
    add("all_0.3", np.full((3, 3), t))
    add("diag_0.3", np.diag([t, t, t]))
    add("mixed_0.3", np.array([[t, 0, t], [0, t, 0], [t, 0, 1.0]]))
    base = np.array([[0.5, 0.125, 0.25], [0.125, 0.75, -0.125], [0.25, -0.125, 1.0]])
    for name, s in (("2^-140", 2.0 ** -140), ("2^-100", 2.0 ** -100), ("2^60", 2.0 ** 60)):
        add(f"scale_{name}", base * s)
        add(f"scale_{name}_rank1", np.outer([1, 2, -1], [1, 2, -1]) * s)
    nan = base.copy(); nan[0, 1] = nan[1, 0] = np.nan
    add("nan_offdiag", nan)
    nan = base.copy(); nan[2, 2] = np.nan
    add("nan_diag", nan)
    inf = base.copy(); inf[0, 0] = np.inf
    add("inf_diag", inf)
    inf = base.copy(); inf[1, 2] = inf[2, 1] = -np.inf
    add("inf_offdiag", inf)
    names = [c[0] for c in cases]
    t6 = [_t6_of(c[1]) for c in cases]
    for i in range(512):
        cnt = int(rng.integers(1, 33))
        v = _unit(rng, (cnt,)) * rng.uniform(0.5, 1.5, (cnt, 1))
        if i % 4 == 0:
            v = v[:1] + 10.0 ** rng.uniform(-7, -1) * rng.standard_normal((cnt, 3))
        T = (v[:, :, None] * v[:, None, :]).sum(0) / (cnt if i % 2 else 1)
        names.append(f"psd{i}")
        t6.append(_t6_of(T))
    with np.errstate(over="ignore", under="ignore"):
        return names, _f32(np.stack(t6))


def _rotations(rng, m):
    q, r = np.linalg.qr(rng.standard_normal((m, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def vu_cases():
    """List of (name, eigval [m,3] ascending, eigvec [m,3,3], n [m,3], tau, damp): every tie pattern of the eigenvalues
    ([a,a,a], [a,a,b], [a,b,b]: the stable descending order decides which COLUMN meets which mask entry), eigenvalues at
    tau and its two float32 neighbours (strict > tau), n = 0, n NaN, and an exact cancellation d n + E^T M E n = 0.
    (E^T M E is positive semi-definite, so with d = 1 no n cancels; the cancelling case uses d = -1, an axis-aligned
    reflected E -- a signed permutation -- all three eigenvalues above tau and n = -e_k: d n = e_k, E^T E n = -e_k.)"""
    rng = _rng("vu")
    tau = F32(0.3)
    lo, hi = np.nextafter(tau, F32(-np.inf)), np.nextafter(tau, F32(np.inf))
    out = []
    m = 64
    E = _rotations(rng, m)
    nrm = _unit(rng, (m,))
    for name, w in (("aaa_above", [0.5, 0.5, 0.5]), ("aaa_below", [0.1, 0.1, 0.1]), ("aab_split", [0.1, 0.1, 0.5]),
                    ("aab_above", [0.4, 0.4, 0.5]), ("abb_split", [0.1, 0.5, 0.5]), ("abb_above", [0.4, 0.5, 0.5]),
                    ("aaa_at_tau", [tau, tau, tau]), ("at_tau", [0.1, tau, 0.5]), ("below_tau", [0.1, lo, 0.5]),
                    ("above_tau", [0.1, hi, 0.5]), ("top_at_tau", [0.1, 0.2, tau]), ("top_above_tau", [0.1, lo, hi]),
                    ("bottom_above_tau", [hi, 0.5, 0.6]), ("tie_at_tau_hi", [tau, hi, hi]), ("tie_lo_tau", [lo, lo, tau])):
        out.append((name, np.tile(_f32(w), (m, 1)), _f32(E), _f32(nrm), 0.3, 3.0))
    out.append(("n_zero", np.tile(_f32([0.1, 0.4, 0.5]), (m, 1)), _f32(E), np.zeros((m, 3), F32), 0.3, 3.0))
    out.append(("n_nan", np.tile(_f32([0.1, 0.4, 0.5]), (m, 1)), _f32(E), np.full((m, 3), np.nan, F32), 0.3, 3.0))
    nn = _f32(nrm); nn[::2, 1] = np.nan
    out.append(("n_nan_component", np.tile(_f32([0.1, 0.4, 0.5]), (m, 1)), _f32(E), nn, 0.3, 3.0))
    perms = list(itertools.permutations(range(3)))
    Es, ns = [], []
    for i, (pm, sg) in enumerate(itertools.product(perms, itertools.product([-1.0, 1.0], repeat=3))):
        P = np.zeros((3, 3))
        for r in range(3):
            P[r, pm[r]] = sg[r]
        Es.append(P)
        ns.append(-np.eye(3)[i % 3])
    out.append(("cancel", np.tile(_f32([0.4, 0.5, 0.6]), (len(Es), 1)), _f32(np.stack(Es)), _f32(np.stack(ns)),
                0.3, -1.0))
    out.append(("cancel_ties", np.tile(_f32([0.5, 0.5, 0.5]), (len(Es), 1)), _f32(np.stack(Es)), _f32(np.stack(ns)),
                0.3, -1.0))
    return out


CLASS_SCALES = (0.2, 0.0, 1.0)


def class_cases():
    """(names, eigval float32 [m, 3] ascending (l3, l2, l1)): all zero (0/0: NaN features, class 0), exact ties of the
    three scores (scale pla == lin for each of CLASS_SCALES, lin == sph, all three equal), a small negative l3,
    l1 = inf, NaN in each slot, and 256 random triples."""
    rng = _rng("classes")
    rows = [("zero", [0, 0, 0]), ("lin==sph", [0.25, 0.5, 1.0]), ("all_equal@scale1", [0.25, 0.5, 0.75]),
            ("pla==lin@scale1", [0.0, 0.5, 1.0]), ("pla==lin==0@scale0", [0.25, 0.25, 1.0]),
            ("sph==0==lin", [0.0, 0.0, 1.0]), ("identity", [1.0, 1.0, 1.0]),
            ("negative_l3", [-1e-9, 0.3, 1.0]), ("negative_l3_flat", [-1e-9, 1e-9, 1.0]),
            ("l1_inf", [0.1, 0.2, np.inf]), ("all_inf", [np.inf] * 3),
            ("nan_l3", [np.nan, 0.5, 1.0]), ("nan_l2", [0.25, np.nan, 1.0]), ("nan_l1", [0.25, 0.5, np.nan]),
            ("l1_zero_l3_negative", [-1.0, -0.5, 0.0]), ("subnormal", [1e-45, 2e-45, 3e-45])]
    # scale * pla == lin at scale = float32(0.2): search the float32 neighbours of l2 = 1/6 (l1 = 1, l3 = 0)
    cand = F32(1.0 / 6.0) + (np.arange(-100, 101) * np.spacing(F32(1.0 / 6.0))).astype(F32)
    tie = cand[(F32(0.2) * ((F32(1) - cand) / F32(1))).astype(F32) == ((cand - F32(0)) / F32(1))]
    assert len(tie), "no float32 l2 ties 0.2 * planarity with linearity"
    rows += [(f"0.2pla==lin#{i}", [0.0, float(t), 1.0]) for i, t in enumerate(tie[:3])]
    names = [r[0] for r in rows]
    w = [np.array(r[1], np.float64) for r in rows]
    for i in range(256):
        w.append(np.sort(rng.random(3) * (10.0 ** rng.uniform(-3, 3))))
        names.append(f"random{i}")
    with np.errstate(under="ignore"):
        return names, _f32(np.stack(w))


# --------------------------------------------------------------------------------------------------------- steps
STEP_KINDS = ("flat", "edge", "feature", "corner", "new", "dummy")


def _dyadic(rng, shape, bits=6, span=2):
    return rng.integers(-span * 2 ** bits, span * 2 ** bits + 1, shape) / 2.0 ** bits


def _dyadic_units(rng, m):
    """Normals with short dyadic components (not unit: the solves do not ask for it)."""
    v = rng.integers(-8, 9, (m, 3)) / 8.0
    v[(v == 0).all(1)] = [0.0, 0.0, 1.0]
    return v


def _case(name, pos, n, ev, ci, lens, nbr, d, alpha, singular=None, **extra):
    lens = np.asarray(lens, np.int64)
    c = dict(name=name, pos=_f32(pos), n=_f32(n), ev=_f32(ev), ci=np.asarray(ci, np.int64), off=_csr(lens),
             nbr=np.asarray(nbr, np.int64).reshape(-1), d=float(d), alpha=float(alpha),
             singular=None if singular is None else np.asarray(singular, bool))
    assert len(c["ci"]) == len(lens) and len(c["nbr"]) == c["off"][-1]
    c.update(extra)
    return c


RAGGED = (0, 1, 2, 3, 8, 31, 64, 65, 200)


def _ragged(rng, npts, lens):
    """Selection rows of the given lengths over npts points: ci distinct, members random (the centre first)."""
    ci = rng.permutation(npts)[:len(lens)]
    nbr = []
    for c, k in zip(ci, lens):
        row = rng.integers(0, npts, k)
        if k:
            row[0] = c
        nbr.append(row)
    return ci, np.concatenate(nbr) if nbr else np.zeros(0, np.int64)


def _clamp_cases(kind, out):
    """A system whose solution is exactly (3, 4, 0) 2^-4 from v_i = 0, so |di| = 5 2^-4 |alpha| exactly: run with d at
    that length and at the next float32 above it, at alpha = 1, 0.5, 0 and -1 (strict < for edge, feature, corner)."""
    h = 2.0 ** -4
    pos = np.zeros((4, 3)); n = np.zeros((4, 3)); ev = np.zeros((4, 3))
    n[1], n[2], n[3] = [1, 0, 0], [0, 1, 0], [0, 0, 1]
    if kind == "corner":            # A = I, b = (v1x, v2y, v3z)
        pos[1], pos[2], pos[3] = [3 * h, 1, -2], [0.5, 4 * h, 1], [-1, 2, 0]
        nbr = [1, 2, 3]
    elif kind == "edge":            # y = e_z: A = diag(1, 1, 2), b = (v1x, v2y, 0)
        ev[0] = [0, 0, 1]
        pos[1], pos[2] = [3 * h, 1, 0.5], [0.5, 4 * h, -1]
        nbr = [1, 2]
    else:                           # feature, n_i = 0: A = I + sum n_j n_j^T = 2 I, b = (v1x, v2y, v3z)
        pos[1], pos[2], pos[3] = [6 * h, 1, -2], [0.5, 8 * h, 1], [-1, 2, 0]
        nbr = [1, 2, 3]
    d0 = F32(5 * h)
    for alpha in (1.0, 0.5, 0.0, -1.0):
        for tag, d in (("at", d0), ("above", np.nextafter(d0, F32(np.inf)))):
            moves = abs(alpha) * 5 * h < float(d)
            out.append(_case(f"clamp_alpha{alpha}_{tag}", pos, n, ev, [0], [len(nbr)], nbr, d, alpha,
                             expect=_f32([[3 * h * alpha, 4 * h * alpha, 0.0]]) if moves else np.zeros((1, 3), F32)))


def step_cases(kind):
    """The selections of one step kind (dicts: name, pos, n, ev, ci, off, nbr, d, alpha, singular [m] = the rows whose
    system has an exactly zero pivot (None where rounding decides whether a rank-deficient system has one), expect
    = the analytic output where there is one). Coordinates and normals are short dyadic numbers: the zero pivots
    are exact."""
    rng = _rng(f"steps_{kind}")
    out = []
    npts = 400
    pos = _dyadic(rng, (npts, 3))
    n = _dyadic_units(rng, npts)
    ev = _dyadic_units(rng, npts)
    lens = list(RAGGED) + [8] * 40
    ci, nbr = _ragged(rng, npts, lens)
    L = np.asarray(lens)
    ez = np.tile([0.0, 0.0, 1.0], (npts, 1))
    if kind == "corner":
        out.append(_case("ragged", pos, n, ev, ci, lens, nbr, 1e6, 1.0))
        out.append(_case("all_ez", pos, ez, ev, ci, lens, nbr, 1e6, 1.0, L >= 0))
        nxz = ez.copy(); nxz[::2] = [1.0, 0.0, 0.0]
        out.append(_case("ex_ez", pos, nxz, ev, ci, lens, nbr, 1e6, 1.0, L >= 0))
        out.append(_case("all_zero", pos, np.zeros((npts, 3)), ev, ci, lens, nbr, 1e6, 1.0, L >= 0))
        out.append(_case("small_d", pos, n, ev, ci, lens, nbr, 0.5, 0.7))
        _clamp_cases(kind, out)
    elif kind == "edge":
        out.append(_case("ragged", pos, n, ev, ci, lens, nbr, 1e6, 0.2))
        out.append(_case("y_ez_n_ez", pos, ez, ez, ci, lens, nbr, 1e6, 0.2, L >= 0))
        out.append(_case("y_zero", pos, n, np.zeros((npts, 3)), ci, lens, nbr, 1e6, 0.2))
        out.append(_case("small_d", pos, n, ev, ci, lens, nbr, 0.5, 0.7))
        _clamp_cases(kind, out)
    elif kind == "feature":
        out.append(_case("ragged", pos, n, ev, ci, lens, nbr, 1e6, 1.0))
        out.append(_case("small_d", pos, n, ev, ci, lens, nbr, 0.5, 0.7))
        out.append(_case("all_zero", pos, np.zeros((npts, 3)), ev, ci, lens, nbr, 1e6, 1.0))
        _clamp_cases(kind, out)
    elif kind in ("flat", "new"):
        un = _unit(rng, (npts,))
        un = un + 0.2 * un[rng.integers(0, npts, npts)]          # correlated, roughly unit normals
        out.append(_case("ragged", pos, un, ev, ci, lens, nbr, 1e6, 1.0))
        out.append(_case("small_d", pos, un, ev, ci, lens, nbr, 0.25, 0.7))
        for d in (0.0, -1.0, np.inf):
            out.append(_case(f"d={d}", pos, un, ev, ci, lens, nbr, d, 1.0))
        if kind == "flat":
            # two neighbours mirrored about the normal: equal weights, di = (0, 0, h) alpha exactly; <= accepts at d = h
            h = 2.0 ** -4
            p = np.array([[0, 0, 0], [0.25, 0, h], [-0.25, 0, h]])
            nn = np.tile([0.0, 0.0, 1.0], (3, 1))
            for tag, d, moves in (("at", F32(h), True), ("below", np.nextafter(F32(h), F32(0)), False)):
                out.append(_case(f"clamp_{tag}", p, nn, nn, [0], [2], [1, 2], d, 1.0,
                                 expect=_f32([[0, 0, h]]) if moves else np.zeros((1, 3), F32)))
    else:
        out.append(_case("ragged", pos, n, ev, ci, lens, nbr, 1.0, 1.0, expect=_f32(pos)[ci]))
    if kind != "dummy":
        # delta = 0: every neighbour of the selection is one point (the centres are others, and that point itself)
        m = 6
        one = np.full(8 * m, 7)
        c0 = np.array([7, 1, 2, 3, 4, 5])
        out.append(_case("delta0", pos, n if kind not in ("flat", "new") else un, ev, c0, [8] * m, one, 1e6, 1.0))
        # one neighbour with a NaN position (point 9), in two of the rows; a NaN centre in a third
        pn = pos.copy(); pn[9] = np.nan
        ci2, nbr2 = _ragged(rng, npts, [8] * 12)
        ci2[ci2 == 9] = 10
        nbr2 = nbr2.reshape(12, 8); nbr2[nbr2 == 9] = 11
        nbr2[:, 0] = ci2
        nbr2[2, 3] = nbr2[5, 7] = 9
        ci2[8] = 9; nbr2[8, 0] = 9
        out.append(_case("nan_position", pn, n if kind not in ("flat", "new") else un, ev, ci2, [8] * 12, nbr2, 1e6,
                         1.0, nan_rows=np.array([2, 5, 8])))
    return out


def _groups(off):
    lens = np.diff(off)
    for k in np.unique(lens):
        rows = np.nonzero(lens == k)[0]
        yield rows, (off[rows][:, None] + np.arange(k)[None, :]).astype(np.int64)


def device_delta(pos, nbr):
    """The global centre and delta of flat / new as the kernels reduce them: centre = float64 mean of every row v_j cast
    to float32, delta = the largest float32 |v_j - centre| with fmaxf's rule (a NaN distance is dropped; nobody: 0)."""
    rows = _f32(pos)[np.asarray(nbr).reshape(-1)]
    with np.errstate(all="ignore"):
        c = (rows.astype(np.float64).sum(0) / max(len(rows), 0)).astype(F32) if len(rows) else np.full(3, np.nan, F32)
        d = rows - c
        dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2]).astype(F32))
    dist = dist[~np.isnan(dist)]
    return c, float(dist.max()) if len(dist) else 0.0


def oracle_step(kind, c, delta=None):
    """oracle/pcd_oracle.py's float32 step on a ragged case: rows grouped by length (the oracle takes dense rows);
    flat / new with ONE global delta over the whole selection (the oracle's own, or the one given)."""
    from oracle import pcd_oracle as O
    pos, n, ev = c["pos"], c["n"], c["ev"]
    out = np.empty((len(c["ci"]), 3), F32)
    with np.errstate(all="ignore"):
        if kind in ("flat", "new") and delta is None:
            delta = O.global_centre_delta(pos, c["nbr"])[1] if len(c["nbr"]) else F32(np.nan)
        for rows, idx in _groups(c["off"]):
            ci, nb = c["ci"][rows], c["nbr"][idx] if idx.size else np.zeros((len(rows), 0), np.int64)
            if kind == "flat":
                out[rows] = O.flat_step(pos, n, ci, nb, c["d"], c["alpha"], delta)
            elif kind == "new":
                out[rows] = O.new_step(pos, n, ci, nb, c["d"], c["alpha"], delta)
            elif kind == "feature":
                out[rows] = O.feature_step(pos, n, ci, nb, c["d"], c["alpha"])
            elif kind == "corner":
                out[rows] = O.corner_step(pos, n, ci, nb, c["d"], c["alpha"])
            elif kind == "edge":
                out[rows] = O.edge_step(pos, n, ev, ci, nb, c["d"], c["alpha"])
            else:
                out[rows] = pos[ci]
    return out


def oracle_ok(kind, c):
    """inv_ex's `info == 0` per row on the system the oracle's corner / edge / feature step builds (the same
    expressions as oracle/pcd_oracle.py, regrouped by row length)."""
    from oracle import pcd_oracle as O
    pos, n, ev = c["pos"], c["n"], c["ev"]
    ok = np.ones(len(c["ci"]), bool)
    with np.errstate(all="ignore"):
        for rows, idx in _groups(c["off"]):
            ci = c["ci"][rows]
            nb = c["nbr"][idx] if idx.size else np.zeros((len(rows), 0), np.int64)
            nj = n[nb]
            if kind == "corner":
                A = (nj[..., :, None] * nj[..., None, :]).sum(1)
            elif kind == "edge":
                y = ev[ci][:, None, :]
                njp = nj - (nj * y).sum(-1, keepdims=True) * y
                A = (njp[..., :, None] * njp[..., None, :] + y[..., :, None] * y[..., None, :]).sum(1)
            else:
                ni = n[ci]
                ni_o = ni[:, :, None] * ni[:, None, :]
                A = (np.eye(3, dtype=F32)[None] + ni_o) + (nj[..., :, None] * nj[..., None, :]).sum(1) \
                    + F32(nb.shape[1]) * ni_o
            ok[rows] = O.inv_ex(A.astype(F32))[1]
    return ok


def step_f64(kind, c):
    """The step formulas of oracle/pcd_oracle.py evaluated in float64 on the float32 inputs (global centre and delta
    included).  A system without an inverse, a non-finite step or one past the clamp keeps v_i.  Sizes the allowance of
    the flat / new comparison only."""
    pos, n, ev = (c[x].astype(np.float64) for x in ("pos", "n", "ev"))
    d, alpha = float(F32(c["d"])), float(F32(c["alpha"]))
    out = pos[c["ci"]].copy()
    with np.errstate(all="ignore"):
        rows_all = pos[c["nbr"]]
        centre = rows_all.mean(0) if len(rows_all) else np.full(3, np.nan)
        delta = np.sqrt(((rows_all - centre) ** 2).sum(1)).max() if len(rows_all) else np.nan
        for r in range(len(c["ci"])):
            i = c["ci"][r]
            nb = c["nbr"][c["off"][r]:c["off"][r + 1]]
            vi, ni, vj, nj = pos[i], n[i], pos[nb], n[nb]
            if kind == "flat":
                W = np.exp(-16 * ((ni - nj) ** 2).sum(1) / delta ** 2) * np.exp(-4 * ((vj - vi) ** 2).sum(1) / delta ** 2)
                di = ((W * (nj * (vj - vi)).sum(1))[:, None] * ni).sum(0) / W.sum() * alpha
                if np.sqrt((di * di).sum()) <= d:
                    out[r] = vi + di
                continue
            if kind == "dummy":
                continue
            if kind == "corner":
                A = (nj[:, :, None] * nj[:, None, :]).sum(0)
                b = (nj * (nj * vj).sum(1)[:, None]).sum(0)
            elif kind == "edge":
                y = ev[i]
                vjp = vj - ((vj - vi) @ y)[:, None] * y
                njp = nj - (nj @ y)[:, None] * y
                A = (njp[:, :, None] * njp[:, None, :]).sum(0) + len(nb) * np.outer(y, y)
                b = (njp * (njp * vjp).sum(1)[:, None]).sum(0) + len(nb) * y * (y @ vi)
            else:
                w = np.ones(len(nb))
                if kind == "new":
                    dot = (nj * (vj - vi)).sum(1)
                    w = np.exp(-9 * dot * dot / delta ** 2)
                nio = np.outer(ni, ni)
                A = np.eye(3) + nio + (w[:, None, None] * nj[:, :, None] * nj[:, None, :]).sum(0) + len(nb) * nio
                b = vi + nio @ vi + nio @ (w[:, None] * vj).sum(0) + (w[:, None] * nj * (nj * vj).sum(1)[:, None]).sum(0)
            if not np.isfinite(A).all() or abs(np.linalg.det(A)) == 0:
                continue
            di = (np.linalg.solve(A, b) - vi) * alpha
            if np.sqrt((di * di).sum()) < d:
                out[r] = vi + di
    return out, centre, delta


def flat_new_allowance(kind, c, got, oracle=None):
    """(ratio, bound) of the flat / new comparison: per row |got - step_f64| against 8 x the largest deviation of the
    float32 oracle from step_f64 in this case + 4u |v_i| (the 8: this suite's allowance over the reference's own
    float32 deviation).  ratio = max row deviation / bound (<= 1 passes)."""
    ref64 = step_f64(kind, c)[0]
    oracle = oracle_step(kind, c) if oracle is None else oracle
    with np.errstate(all="ignore"):
        own = np.abs(oracle.astype(np.float64) - ref64)
        own = own[np.isfinite(own)]
        bound = 8.0 * (own.max() if len(own) else 0.0) + 4 * U * np.sqrt((ref64 ** 2).sum(1))
        dev = np.abs(np.asarray(got, np.float64) - ref64).max(1)
    fin = np.isfinite(ref64).all(1)
    ratio = float((dev[fin] / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0
    return ratio, dev, bound, fin


# ------------------------------------------------------------------------------------------ shared by both test files
def vote_cases():
    """(label, rho, rows = (pos, n, ci, off, nbr), may [E] bool: the pairs that are allowed to be undecided) over every
    vote builder at every rho of RHOS and SPECIAL_RHOS."""
    for rho in RHOS + SPECIAL_RHOS:
        tag = f"rho={float(F32(rho)):.4f}"
        # rho = pi/2 puts the threshold at c = 0: the perpendicular, zero-normal and clamped tiny pairs of every builder
        # sit on it, so there (and only there) the pairs with c64 <= 1e-6 may be undecided as well
        at_zero = (lambda rows: pair_c64(*rows[:5]) <= 1e-6) if rho == math.pi / 2 else \
            (lambda rows: np.zeros(len(rows[4]), bool))
        for unit in (True, False):
            rows = threshold_rows(rho, unit)
            yield f"threshold[{'unit' if unit else 'nonunit'}] {tag}", rho, rows, np.ones(len(rows[4]), bool)
        rows = scale_rows(rho)
        yield f"scale {tag}", rho, rows[:5], rows[5] | at_zero(rows)
        rows = fallback_rows(exact=rho == 0)
        yield f"fallback {tag}", rho, rows, at_zero(rows)
        rows = odd_normal_rows()
        # (a NaN normal at rho < 0: the two clips differ, see vote_judge)
        yield f"odd_normals {tag}", rho, rows, (np.isnan(rows[1][rows[4]]).any(1) & (rho < 0)) | at_zero(rows)


def judge_rows(rho, rows, may, kind="nvt"):
    """The judge and the candidates of one vote case, with the caps every builder must meet: no unjudged row, no
    undecided pair outside `may`."""
    pos, n, ci, off, nbr = rows
    state = vote_judge(pos, n, ci, off, nbr, rho) if kind == "nvt" else normal_vote_judge(n, ci, off, nbr, rho)
    cands = admissible_decompositions(n, (off, nbr), state, kind, pos, ci)
    assert len(cands["unjudged"]) == 0, f"{len(cands['unjudged'])} rows with more than {MAX_U} undecided pairs"
    stray = (state == UNDECIDED) & ~np.asarray(may, bool)
    assert not stray.any(), f"{stray.sum()} undecided pairs where none may be: {np.nonzero(stray)[0][:8]}"
    return state, cands


def check_decompositions(label, cands, m, eigval, eigvec, t6=None):
    """Every row bit-equal (NaN pattern included) to one admissible candidate.  -> a line for the report."""
    pairs = [(eigval, "eigval"), (eigvec, "eigvec")] + ([(t6, "t6")] if t6 is not None else [])
    ok, taken = match_candidates(cands, m, *pairs)
    und = np.nonzero(cands["u"] > 0)[0]
    hist = np.bincount(taken[und][taken[und] >= 0], minlength=1)
    assert ok.all(), (f"{label}: {(~ok).sum()} of {m} rows match no admissible candidate, first rows "
                      f"{np.nonzero(~ok)[0][:8]}; row {np.nonzero(~ok)[0][0]} got eigval "
                      f"{np.asarray(eigval)[np.nonzero(~ok)[0][0]]}, candidates "
                      f"{cands['eigval'][cands['row'] == np.nonzero(~ok)[0][0]]}")
    return f"{label}: {m} rows all admissible (bound: all), {len(und)} with undecided pairs, candidate taken {hist.tolist()}"


# ------------------------------------------------------------------------------------ the fused loop on hard clouds
FUSED_CLOUDS = ("sheet", "line", "plane_exact", "point", "needle", "two_clusters", "lattice_ties", "tiny_values",
                "translated")
FUSED_RHO = 5 * math.pi / 12


def hard_cloud(name):
    """(pos, n): the snapshot of knn_ref.CASES[name] with seeded unit normals -- e_z on plane_exact, e_z tilted by a
    seeded 0.2 rad on sheet (the clouds with a surface), random directions elsewhere."""
    import knn_ref
    pos = knn_ref.CASES[name]()[0]
    rng = _rng("normals_" + name)
    if name == "plane_exact":
        n = np.tile([0.0, 0.0, 1.0], (len(pos), 1))
    elif name == "sheet":
        n = np.array([0.0, 0.0, 1.0]) + 0.2 * rng.standard_normal((len(pos), 3))
    else:
        n = rng.standard_normal((len(pos), 3))
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return _f32(pos), _f32(n)


def dense_csr(lists):
    m, k = lists.shape
    return np.arange(m), np.arange(m + 1, dtype=np.int64) * k, np.ascontiguousarray(lists, np.int64).reshape(-1)


def nvt_stage(pos, n, lists, rho=FUSED_RHO, smooth=None):
    """The judge and the candidates of one NVT stage over dense lists; smooth = (n, tau, damp): each candidate's VU
    smoothed normal as field "fn".  Every candidate also carries its classes ("cls") and edge vector ("edge")."""
    from oracle import pcd_oracle as O
    ci, off, nbr = dense_csr(lists)
    state = vote_judge(pos, n, ci, off, nbr, rho)
    cands = admissible_decompositions(n, (off, nbr), state)
    with np.errstate(all="ignore"):
        if smooth is not None:
            cands["fn"] = O.vu_smoothed_normals(cands["eigval"], cands["eigvec"], _f32(smooth[0])[cands["row"]],
                                                smooth[1], smooth[2])
        cands["cls"] = O.classes(cands["eigval"])
        cands["edge"] = np.ascontiguousarray(cands["eigvec"][..., 0])
    return state, cands


def class_margin(eigval, scale=0.2):
    from oracle import pcd_oracle as O
    with np.errstate(all="ignore"):
        p, l, s = O.nvt_features(_f32(eigval))
        f = np.sort(np.stack([F32(scale) * p, l, s], 1), 1)
        return f[:, 2] - f[:, 1]


def fused_reference_caps(name, k):
    """The caps of the fused comparison from the reference alone (knn_ref.knn_f32 lists, the base candidate's chain):
    (fraction of rows with undecided pairs in NVT1, in NVT2, fraction of rows whose class margin is <= 1e-5)."""
    import knn_ref
    pos, n = hard_cloud(name)
    lists, _ = knn_ref.knn_f32(pos, pos, k, np.arange(len(pos)))
    _, c1 = nvt_stage(pos, n, lists, smooth=(n, 0.3, 3.0))
    first = np.unique(c1["row"], return_index=True)[1]
    fn = c1["fn"][first]
    _, c2 = nvt_stage(pos, fn, lists)
    first2 = np.unique(c2["row"], return_index=True)[1]
    margin = class_margin(c2["eigval"][first2])
    return float((c1["u"] > 0).mean()), float((c2["u"] > 0).mean()), float(np.mean(~(margin > 1e-5)))
