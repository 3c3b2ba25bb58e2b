"""GPU tests of the sparse-PCA solver kernels themselves (csrc/eofx_spca.hpp) against float64 / longdouble numpy, at the
edges of their shapes: eofx_spca_loop_f64 one iteration at a time, the zero-column completion rule, the batch of 16, the
three helper entries (gram, rowmul, prox) called directly, and spca_svd / spca_orth.

THE ONE-STEP METHOD.  The loop is bitwise deterministic and check = 0 runs exactly max_iter iterations, so runs with
max_iter = 1, 2, 3 give B_1, B_2, B_3 (B_0 = V[:, :k]), and the run with max_iter = T gives Qa_T (the polar factor update
T used), dtilde_T and objective[T - 1].  Each kernel is then judged on its own, from the state the kernels themselves
produced one step earlier -- no trajectory drift enters:
  polar      M = D^2 (V^T B_{T-1}) from the downloaded B_{T-1} (longdouble sums): Qa^T Qa = I, H = Qa^T M symmetric with
             eigenvalues >= -tol, eig(H) descending = dtilde, Qa H = M.  Per residual the kernel is allowed 10 x
             max(the same residual of numpy's LAPACK polar factor U W^T of the same M, l eps |M|_2); the orthogonality
             residual is scaled by |M|_2 so that all four share one unit.  Where cond(M) <= 1e6, Qa also equals the LAPACK
             factor to 1e-9 relative.
  update     with the kernel's own Qa_T: W = D^2 (Qa_T - P), pre = B + nu (V W - beta2 B), B_T = prox(pre, kappa), compared
             entrywise within (l + 4) 2^-53 (|B| + nu (|V| |W| + beta2 |B|)) + nu |V| D^2 dP.  The first term is the forward
             bound of the update GIVEN W; the second is what the rounding of the kernels' own P (which cannot be
             downloaded) does to W: dP = depth 2^-53 |V|^T |B| with depth = ceil(p / G) + ceil(G / 256) + 8, the additions
             behind one entry of P (a workgroup's rows in order, its thread's partials in order, the tree over 256
             threads).  Without it the check cannot hold for ANY float64 P: the numpy restatement, whose P is a BLAS
             product, misses the first term alone by up to 9x at entries just above the threshold, and so do the kernels
             ("bare" below); with it the kernels stay below a tenth of the bound.  An entry whose reference |pre| lies within
             SAFETY = 1000 x the bound of the threshold (kappa for l1, sqrt(2 kappa) for l0) would be excused; the test
             counts them from the reference alone and asserts the count is 0.  Beyond 1 000 000 entries of B the
             elementwise part of the reference is float64 (4 roundings against the bound's l + 4).
  objective  objective[T - 1] against 1/2 sum_a D_a^2 (|q_a - p'_a|^2 + 1 - |q_a|^2) + alpha2 sum|B_T| + beta2/2 sum B_T^2
             with P' = V^T B_T in longdouble, and against the definition 1/2 |D V^T (I - B_T A^T)|^2 + ..., A = V Qa.
             Tolerance p 2^-53 sum|terms| (terms: the summands above with |q| + |p'| for q - p' and 1 + |q|^2 for
             1 - |q|^2); the definition's also carries l |V^T V - I|_max sum|terms|, the reference V's own departure from
             orthonormality, which the kernel's formula assumes away.
Longdouble sums: products with an inner dimension beyond a few thousand are taken as float64 BLAS products over blocks of
32 (128 beyond 4096) inner indices whose block results are then summed in longdouble -- an error of 32 (128) 2^-53 against
tolerances of a 2^-53 / p 2^-53 with a, p the full inner dimension; everything smaller is longdouble throughout.  The two
l x k / k x p products of the definition at 4 000 000 multiplications and more are plain float64 (inner dimension <= 128
against p >= 488).

SHAPES.  The table of the issue, unshrunk: the slowest case, 70 000 x 128 x 64, took 2.0 s (its host reference, not the
kernels, is the cost) and every other one under a second, so no p was lowered.

MEASURED on an MI355X, per case the largest over T = 1, 2, 3, in units of l eps |M|_2 (kernel / LAPACK, for the four polar
residuals orth, sym, eig, recon, and the most negative eigenvalue "neg" as it is), Qa against the LAPACK factor (nan:
cond(M) > 1e6 at some T), the largest update error as a fraction of its bound (and of its first term alone), the two
objective differences as fractions of their tolerances, and the excused-entry count:
  p1-l1-k1  orth 0/0 sym 0/0 eig 0/0 recon 0/0  neg 0  Qa-LAPACK 0.0e+00  upd 0.041 (bare 0.12)  obj 0.00021 0.00013  excused 0
  p2-l2-k2  orth 0.12/0.11 sym 0.049/0.0079 eig 0.25/0 recon 0.12/0.11  neg 0  Qa-LAPACK 2.8e-17  upd 0.069 (bare 0.32)  obj 0.038 0.00033  excused 0
  p2-l2-k1  orth 0.11/0.11 sym 0/0 eig 0.25/0 recon 0.11/0.11  neg 0  Qa-LAPACK 2.8e-17  upd 0.069 (bare 0.32)  obj 0.13 0.14  excused 0
  p31-l5-k5  orth 0.78/1 sym 0.76/0.39 eig 0.5/0.8 recon 0.78/1  neg 0  Qa-LAPACK 7.9e-16  upd 0.037 (bare 8.9)  obj 0.0026 0.012  excused 0
  p32-l5-k5  orth 1.7/0.97 sym 0.49/0.43 eig 1/1.3 recon 1.7/0.97  neg 0  Qa-LAPACK 1.1e-15  upd 0.035 (bare 4.9)  obj 0.0012 0.04  excused 0
  p33-l5-k5  orth 0.92/0.77 sym 0.24/0.33 eig 0.4/1 recon 0.92/0.77  neg 0  Qa-LAPACK 7.8e-16  upd 0.041 (bare 3.6)  obj 0.0012 0.018  excused 0
  p127-l5-k5  orth 0.65/1.2 sym 0.53/0.61 eig 0.61/0.81 recon 0.65/1.2  neg 0  Qa-LAPACK 6.7e-16  upd 0.026 (bare 5.4)  obj 0.0014 0.0018  excused 0
  p128-l5-k5  orth 0.76/0.9 sym 0.33/0.47 eig 0.5/0.81 recon 0.76/0.9  neg 0  Qa-LAPACK 7.8e-16  upd 0.023 (bare 4.1)  obj 0.00039 0.0043  excused 0
  p129-l5-k5  orth 1.3/1.3 sym 0.28/1.2 eig 0.8/1.4 recon 1.3/1.3  neg 0  Qa-LAPACK 1.2e-15  upd 0.021 (bare 3.6)  obj 0.00088 0.0067  excused 0
  p257-l5-k5  orth 1.3/1.6 sym 0.23/1.7 eig 0.41/1 recon 1.3/1.6  neg 0  Qa-LAPACK 1.3e-15  upd 0.026 (bare 7)  obj 0.00026 0.0049  excused 0
  p300-l7-k1-l1  orth 0.14/0.14 sym 0/0 eig 0.36/0.15 recon 0.14/0.14  neg 0  Qa-LAPACK 2.2e-16  upd 0.031 (bare 0.55)  obj 0.00013 0.00087  excused 0
  p300-l7-k1-l0  orth 0.018/0.3 sym 0/0 eig 0.072/0.21 recon 0.018/0.3  neg 0  Qa-LAPACK 2.2e-16  upd 0.016 (bare 0.2)  obj 0.00017 0.00022  excused 0
  p300-l8-k4-l1  orth 0.51/0.38 sym 0.056/0.014 eig 0.13/0.13 recon 0.11/0.15  neg 0  Qa-LAPACK 7.2e-16  upd 0.086 (bare 1.8)  obj 0.0006 0.0013  excused 0
  p300-l8-k4-l0  orth 0.4/0.8 sym 0.056/0.049 eig 0.31/0.25 recon 0.18/0.39  neg 0  Qa-LAPACK 7.2e-16  upd 0.052 (bare 0.26)  obj 0.0002 0.0014  excused 0
  p300-l8-k8-l1  orth 1.3/1.4 sym 0.89/0.81 eig 0.095/0.25 recon 0.9/0.28  neg 0  Qa-LAPACK 6.7e-15  upd 0.084 (bare 1.3)  obj 0.00047 0.0043  excused 0
  p300-l8-k8-l0  orth 1.1/0.95 sym 0.42/4.5 eig 0.25/0.13 recon 0.42/0.3  neg 0  Qa-LAPACK nan  upd 0.057 (bare 0.27)  obj 0.00082 0.0034  excused 0
  p1000-l128-k30-lds  orth 0.99/0.098 sym 0.7/0.15 eig 0.044/0.08 recon 0.73/0.088  neg 0  Qa-LAPACK 2.3e-14  upd 0.0069 (bare 0.18)  obj 3.2e-05 0.0028  excused 0
  p129-l128-k63-l1  orth 1/0.13 sym 0.8/0.063 eig 0.039/0.15 recon 0.8/0.11  neg 0  Qa-LAPACK 2.8e-14  upd 0.014 (bare 0.89)  obj 0.0013 0.012  excused 0
  p129-l128-k63-l0  orth 1/0.13 sym 0.96/0.031 eig 0.035/0.12 recon 0.96/0.13  neg 0  Qa-LAPACK 2.8e-14  upd 0.014 (bare 0.066)  obj 0.00025 0.012  excused 0
  p4099-l128-k64-l1  orth 1/0.16 sym 0.84/0.077 eig 0.047/0.049 recon 0.85/0.12  neg 0  Qa-LAPACK 2.8e-14  upd 0.011 (bare 0.065)  obj 9.7e-05 0.0021  excused 0
  p4099-l128-k64-l0  orth 1/0.13 sym 0.92/0.077 eig 0.056/0.069 recon 0.92/0.085  neg 0  Qa-LAPACK 2.9e-14  upd 0.0082 (bare 0.023)  obj 5.6e-05 0.0028  excused 0
  p70000-l128-k64-partcap  orth 1/0.14 sym 0.53/0.22 eig 0.068/0.068 recon 0.59/0.091  neg 0  Qa-LAPACK 2.8e-14  upd 0.014 (bare 0.063)  obj 3.7e-06 7.5e-05  excused 0
  p262275-l2-k1-gmax  orth 0.26/1 sym 0/0 eig 0.39/0.41 recon 0.26/1  neg 0  Qa-LAPACK 2.2e-16  upd 0.026 (bare 0.48)  obj 1.5e-06 3.1e-06  excused 0
  p5000-l128-k64-tiny  orth 0.99/0.14 sym 0.78/0.14 eig 0.05/0.13 recon 0.97/0.11  neg 3e-16  Qa-LAPACK nan  upd 0.0035 (bare 0.093)  obj 2.2e-05 0.0019  excused 0
  p300-l16-k4-zeroD  orth 0.81/0.74 sym 0.11/0.058 eig 0.22/0.16 recon 0.44/0.54  neg 0  Qa-LAPACK 1.7e-15  upd 0.021 (bare 1.6)  obj 0.0003 0.0011  excused 0

THE CHECKER IS NOT SLACK (test_checker_rejects_a_wrong_rotation_and_a_wrong_partial, CPU arithmetic only).  The numpy
restatement of the kernels (emulate_loop: the same round-robin one-sided Jacobi, completion rule, update and objective)
passes the one-step checks; with ONE rotation applied to J at an angle off by 1e-6 the symmetry residual of the polar
check exceeds its tolerance by more than 1e3, and with ONE entry of P' off by 1e-6 the objective check exceeds its
tolerance by more than 1e3.
"""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
SENT = -7.25e300            # what untouched host outputs hold
REG = {"l1": 0, "l0": 1}
SAFETY = 1000.0


# ------------------------------------------------------------------------------------------------ numpy side
def hp_matmul(A, B):
    """A B in longdouble (small products), or float64 products over blocks of the inner dimension summed in longdouble"""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    m, n = A.shape
    q = B.shape[1]
    if m * n * q <= 4_000_000:
        return A.astype(LD) @ B.astype(LD)
    blk = 32 if n <= 4096 else 128
    nb = -(-n // blk)
    Bp = np.zeros((nb * blk, q))
    Bp[:n] = B
    Bp = Bp.reshape(nb, blk, q)
    out = np.empty((m, q), LD)
    mc = max(1, 8_000_000 // (nb * q))
    for r0 in range(0, m, mc):
        Ap = np.zeros((min(mc, m - r0), nb * blk))
        Ap[:, :n] = A[r0:r0 + mc]
        part = Ap.reshape(-1, nb, blk).transpose(1, 0, 2) @ Bp
        out[r0:r0 + mc] = part.sum(axis=0, dtype=LD)
    return out


def prox_np(x, reg, kappa):
    """the kernel's prox, operation by operation (any float dtype)"""
    if reg == "l0":
        return np.where(x * x < 2.0 * kappa, 0.0 * x, x)
    a = np.abs(x) - kappa
    return np.where(a > 0.0, np.copysign(a, x), 0.0 * x)


def scaled(D, alpha, beta):
    d0 = float(D[0]) * float(D[0])
    a2, b2 = alpha * d0, beta * d0
    nu = 1.0 / (d0 + b2)
    return a2, b2, nu, nu * a2


def lapack_polar(M):
    Us, s, Wt = np.linalg.svd(M, full_matrices=False)
    return Us @ Wt, s


def completion_columns(basis, count, l):
    """the documented rule: for each missing column in turn the next unit vector e_0, e_1, ... not in the span of the
    columns already there (`basis`: the live ones by descending singular value, then the completed ones) -- two
    Gram-Schmidt passes, accepted when what is left is longer than 1/2"""
    basis = [np.asarray(b, np.float64) for b in basis]
    out, nxt = [], 0
    for _ in range(count):
        while nxt < l:
            u = np.zeros(l)
            u[nxt] = 1.0
            nxt += 1
            for _pass in range(2):
                for b in basis:
                    u = u - (b @ u) * b
            nn = np.sqrt(u @ u)
            if nn > 0.5:
                u = u / nn
                basis.append(u)
                out.append(u)
                break
    return np.array(out).T.reshape(l, len(out))


def jacobi_polar(M, wrong_rotation=0.0):
    """spca_step_kernel's polar step restated: round-robin one-sided Jacobi, the ordering, the completion rule.
    wrong_rotation != 0: the first rotation reaches J at an angle off by that much (a deliberately wrong kernel)."""
    M = np.array(M, np.float64)
    l, k = M.shape
    J = np.eye(k)
    m = k + (k & 1)
    half = m // 2
    eps = EPS * l
    t = np.arange(half)
    for _sweep in range(60):
        if m <= 1:
            break
        rot = False
        for rnd in range(m - 1):
            i1 = np.where(t == 0, rnd, (rnd + t) % (m - 1))
            i2 = np.where(t == 0, m - 1, (rnd - t + m - 1) % (m - 1))
            Pc, Qc = np.minimum(i1, i2), np.maximum(i1, i2)
            Pc, Qc = Pc[Qc < k], Qc[Qc < k]
            x, y = M[:, Pc], M[:, Qc]
            a, b, g = (x * x).sum(0), (y * y).sum(0), (x * y).sum(0)
            do = (g != 0.0) & (np.abs(g) > eps * np.sqrt(a * b))
            if not do.any():
                continue
            rot = True
            Pc, Qc, a, b, g = Pc[do], Qc[do], a[do], b[do], g[do]
            zeta = (b - a) / (2.0 * g)
            with np.errstate(over="ignore"):
                tt = np.where(np.abs(zeta) > 1e150, 0.5 / zeta,
                              np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta)))
            c = 1.0 / np.sqrt(1.0 + tt * tt)
            s = tt * c
            x, y = M[:, Pc].copy(), M[:, Qc].copy()
            M[:, Pc], M[:, Qc] = c * x - s * y, s * x + c * y
            if wrong_rotation:
                th = np.arctan2(s[0], c[0]) + wrong_rotation
                c, s = c.copy(), s.copy()
                c[0], s[0] = np.cos(th), np.sin(th)
                wrong_rotation = 0.0
            x, y = J[:, Pc].copy(), J[:, Qc].copy()
            J[:, Pc], J[:, Qc] = c * x - s * y, s * x + c * y
        if not rot:
            break
    sig = np.sqrt((M * M).sum(0))
    order = sorted(range(k), key=lambda j: (-sig[j], j))
    smax = sig[order[0]]
    live = (sig > 0.0) & (sig > smax * eps)
    Uc = np.where(live, M / np.where(live, sig, 1.0), 0.0)
    dead = [c for c in order if not live[c]]
    if dead:
        Uc[:, dead] = completion_columns([Uc[:, c] for c in order if live[c]], len(dead), l)
    return Uc @ J.T, sig[order]


def objective_np(D2, Qa, P, a2, b2, B):
    r = (((Qa - P) ** 2).sum(axis=1) + (1.0 - (Qa ** 2).sum(axis=1))) @ D2
    return 0.5 * r + a2 * np.abs(B).sum() + 0.5 * b2 * (B * B).sum()


def emulate_loop(V, D, k, alpha=1e-3, beta=1e-3, reg="l1", max_iter=1, tol=0.0, check=0, wrong_rotation=None,
                 wrong_partial=None):
    """eofx_spca_loop_f64 in float64 numpy.  wrong_rotation / wrong_partial = (iteration, size): the polar step before
    that update gets one wrong rotation / one entry of that update's P' is off (for the sanity test of the checker)."""
    D = np.asarray(D, np.float64)
    D2 = D * D
    a2, b2, nu, kappa = scaled(D, alpha, beta)
    B = V[:, :k].copy()
    P = V.T @ B
    obj = []
    for t in range(1, max_iter + 1):
        Qa, dt = jacobi_polar(D2[:, None] * P, wrong_rotation[1] if wrong_rotation and wrong_rotation[0] == t else 0.0)
        W = D2[:, None] * (Qa - P)
        B = prox_np(B + nu * (V @ W - b2 * B), reg, kappa)
        P = V.T @ B
        Po = P.copy()
        if wrong_partial and wrong_partial[0] == t:
            Po[0, 0] += wrong_partial[1]
        obj.append(objective_np(D2, Qa, Po, a2, b2, B))
        if t >= max_iter or (check and t - 1 > 0 and abs(obj[-2] - obj[-1]) / obj[-1] < tol):
            break
    return dict(B=B, Qa=Qa, dtilde=dt, objective=np.array(obj), n_iter=len(obj))


def spca_grid(rows, entries):
    """the workgroups of a streaming pass, as the ABI documents them: about 128 rows each, at most 2048, partials within 32 MiB"""
    return max(1, min(2048, max(1, (rows + 127) // 128), max(1, (4 << 20) // max(1, entries))))


def make_V(p, l, seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((p, l)), mode="reduced")[0]


def spectrum(kind, l, k):
    if kind == "flat":
        return np.ones(l)
    if kind in ("dec3", "dec6"):
        return np.logspace(0.0, -3.0 if kind == "dec3" else -6.0, l)
    D = np.logspace(0.0, -1.0, l)
    if kind == "tiny":
        D[k - 2:] = 1e-9 * D[0]
    elif kind == "zero8":
        D[8:] = 0.0
    else:
        raise ValueError(kind)
    return D


def polar_residuals(Q, dt, M, nM):
    k = M.shape[1]
    Ql, Ml = Q.astype(LD), M.astype(LD)
    H = Ql.T @ Ml
    w = np.linalg.eigvalsh(np.asarray(0.5 * (H + H.T), np.float64))[::-1]
    return dict(orth=float(np.abs(Ql.T @ Ql - np.eye(k)).max()) * nM, sym=float(np.abs(H - H.T).max()),
                neg=max(0.0, -float(w.min())), eig=float(np.abs(w - dt).max()), recon=float(np.abs(Ql @ H - Ml).max()))


def check_steps(V, D, k, alpha, beta, reg, runs):
    """the one-step checks of the module docstring on runs = {T: outputs of the loop with max_iter = T}, T = 1 .. n (all
    present).  -> (figures per T, list of failures)"""
    p, l = V.shape
    D = np.asarray(D, np.float64)
    D2 = D * D
    a2, b2, nu, kappa = scaled(D, alpha, beta)
    thr = kappa if reg == "l1" else np.sqrt(2.0 * kappa)
    absV = np.abs(V)
    G = spca_grid(p, l * k + 2)
    depth = -(-p // G) + -(-G // 256) + 8           # additions behind one entry of P: the rows of a workgroup, its thread's partials, the tree
    vdef = float(np.abs(hp_matmul(V.T, V) - np.eye(l)).max())
    Bs = {0: V[:, :k].copy()}
    Bs.update({T: runs[T]["B"] for T in runs})
    Pld = {T: hp_matmul(V.T, Bs[T]) for T in Bs}
    figs, fails = {}, []
    for T in sorted(runs):
        out, Bp, Bt = runs[T], Bs[T - 1], Bs[T]
        Qa, dt = out["Qa"], out["dtilde"]
        f = figs[T] = {}
        # ---- polar
        M = np.asarray(D2[:, None] * Pld[T - 1], np.float64)
        sv = np.linalg.svd(M, compute_uv=False)
        nM = float(sv[0])
        floor = l * EPS * nM
        Ql, sl = lapack_polar(M)
        got, lap = polar_residuals(Qa, dt, M, nM), polar_residuals(Ql, sl, M, nM)
        f["polar"] = {key: (got[key], lap[key], 10.0 * max(lap[key], floor)) for key in got}
        f["floor"] = floor
        for key, (g, _, tol) in f["polar"].items():
            if not g <= tol:
                fails.append(f"T={T} polar {key}: {g:.3e} > {tol:.3e} (x{g / tol:.1e})")
        f["cond"] = float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf
        f["polar_q"] = None
        if f["cond"] <= 1e6:
            f["polar_q"] = float(np.abs(Qa - Ql).max() / np.abs(Ql).max())
            if not f["polar_q"] <= 1e-9:
                fails.append(f"T={T} Qa vs LAPACK polar: {f['polar_q']:.3e} > 1e-9")
        # ---- update
        W = np.asarray(D2[:, None].astype(LD) * (Qa.astype(LD) - Pld[T - 1]), np.float64)
        VW = hp_matmul(V, W)
        if p * k <= 1_000_000:
            pre = Bp.astype(LD) + LD(nu) * (VW - LD(b2) * Bp.astype(LD))
            kap, th = LD(kappa), LD(thr)
        else:                           # elementwise float64 beyond that: 4 roundings of the reference against the bound's l + 4
            pre = Bp + nu * (np.asarray(VW, np.float64) - b2 * Bp)
            kap, th = kappa, thr
        bound0 = (l + 4) * U * (np.abs(Bp) + nu * (absV @ np.abs(W) + b2 * np.abs(Bp)))
        bound = bound0 + nu * (absV @ (D2[:, None] * (depth * U) * (absV.T @ np.abs(Bp))))      # + what P's own rounding does to W
        f["excused"] = int(np.count_nonzero(np.abs(np.asarray(np.abs(pre) - th, np.float64)) <= SAFETY * bound))
        if f["excused"]:
            fails.append(f"T={T} {f['excused']} entries within {SAFETY:g} x the bound of the threshold: choose another seed")
        err = np.abs(np.asarray(Bt - prox_np(pre, reg, kap), np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / bound)
            f["upd0"] = float(np.where(err == 0.0, 0.0, err / bound0).max())
        f["upd"] = float(ratio.max())
        if not f["upd"] <= 1.0:
            fails.append(f"T={T} update: {int((ratio > 1).sum())} entries beyond the forward bound, worst x{f['upd']:.2e}")
        # ---- objective
        o = float(out["objective"][T - 1])
        Pn, Ql_ = Pld[T], Qa.astype(LD)
        D2l = D2.astype(LD)
        reg_terms = LD(a2) * np.abs(Bt).sum(dtype=LD) + LD(0.5 * b2) * (Bt.astype(LD) ** 2).sum()
        o1 = LD(0.5) * (D2l * (((Ql_ - Pn) ** 2).sum(axis=1) + 1.0 - (Ql_ ** 2).sum(axis=1))).sum() + reg_terms
        terms = float(LD(0.5) * (D2l * (((np.abs(Ql_) + np.abs(Pn)) ** 2).sum(axis=1) + 1.0 + (Ql_ ** 2).sum(axis=1))).sum()
                      + reg_terms)
        DVt = np.ascontiguousarray((V * D).T)
        if p * l * k > 4_000_000:       # float64 for the two products of inner dimension k and l (see the module docstring)
            R = DVt - np.asarray(D[:, None] * Pn, np.float64) @ (V @ Qa).T
            o2 = LD(0.5) * (R * R).sum(dtype=LD) + reg_terms
        else:
            R = DVt.astype(LD) - (D[:, None] * Pn) @ hp_matmul(V, Qa).T
            o2 = LD(0.5) * (R ** 2).sum() + reg_terms
        tol1 = p * U * terms
        tol2 = tol1 + l * vdef * terms
        f["obj1"], f["obj2"] = (abs(float(o - o1)), tol1), (abs(float(o - o2)), tol2)
        for key in ("obj1", "obj2"):
            d, tol = f[key]
            if not d <= tol:
                fails.append(f"T={T} {key}: |{o!r} - reference| = {d:.3e} > {tol:.3e} (x{d / tol:.1e})")
    return figs, fails


def figure_line(name, figs):
    """one line of the docstring's table: the largest figures over T"""
    w = lambda key, i: max(f["polar"][key][i] / f["floor"] if f["floor"] > 0 else 0.0 for f in figs.values())
    pol = " ".join(f"{key} {w(key, 0):.2g}/{w(key, 1):.2g}" for key in ("orth", "sym", "eig", "recon"))
    neg = max(f["polar"]["neg"][0] for f in figs.values())
    qs = [f["polar_q"] for f in figs.values() if f["polar_q"] is not None]
    return (f"  {name:<26s} {pol}  neg {neg:.1g}  Qa-LAPACK {max(qs) if qs else float('nan'):.1e}  "
            f"upd {max(f['upd'] for f in figs.values()):.2g} (bare {max(f['upd0'] for f in figs.values()):.2g})  "
            f"obj {max(f['obj1'][0] / f['obj1'][1] for f in figs.values()):.2g} "
            f"{max(f['obj2'][0] / f['obj2'][1] for f in figs.values()):.2g}  "
            f"excused {sum(f['excused'] for f in figs.values())}")


# ------------------------------------------------------------------------------------------------ device side
@pytest.fixture(scope="module")
def ctx():
    from xeofs_amd import engine

    return engine.default_context()


def dev(ctx, a):
    from xeofs_amd import spca

    return spca._dev64(ctx, np.ascontiguousarray(a, dtype=np.float64))


def dev1(ctx, a):
    """a float64 device vector"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(f"cuda:{ctx.device}")


def last_error(ctx):
    return ctx.lib.eofx_last_error(ctx.handle).decode(errors="replace")


def loop_raw(ctx, Vd, D, k, alpha=1e-3, beta=1e-3, reg=0, max_iter=1, tol=0.0, check=0, want_obj=True, pad=4, p=None, l=None):
    """eofx_spca_loop_f64 as spca_solve calls it -> (status, outputs); host outputs are pre-filled with SENT"""
    import torch

    from xeofs_amd._lib import ptr

    p = Vd.shape[0] if p is None else p
    l = Vd.shape[1] if l is None else l
    D = np.ascontiguousarray(D, dtype=np.float64)
    if isinstance(Vd, np.ndarray):
        B = torch.zeros((p, max(k, 1)), dtype=torch.float64, device=ctx.device)
    else:
        B = torch.full((p, max(k, 1)), float("nan"), dtype=torch.float64, device=Vd.device)
    Qa = np.full((l, max(k, 1)), SENT)
    dt = np.full(max(k, 1), SENT)
    obj = np.full(max(int(max_iter), 0) + pad, SENT) if want_obj else None
    it = C.c_int(-1)
    rc = ctx.lib.eofx_spca_loop_f64(ctx.handle, ptr(Vd), p, l, ptr(D), k, float(alpha), float(beta), int(reg), int(max_iter),
                                    float(tol), int(check), ptr(B), ptr(Qa), ptr(dt), ptr(obj), C.byref(it))
    return rc, dict(B=B, Qa=Qa, dtilde=dt, objective=obj, n_iter=it.value)


def loop(ctx, Vd, D, k, alpha=1e-3, beta=1e-3, reg="l1", **kw):
    from xeofs_amd._lib import raise_for

    rc, out = loop_raw(ctx, Vd, D, k, alpha, beta, REG[reg], **kw)
    raise_for(rc, ctx.handle)
    out["B"] = out["B"].cpu().numpy()
    return out


def same_state(a, b, n):
    return (np.array_equal(a["B"], b["B"]) and np.array_equal(a["Qa"], b["Qa"]) and np.array_equal(a["dtilde"], b["dtilde"])
            and np.array_equal(a["objective"][:n], b["objective"][:n]))


# ------------------------------------------------------------------------------------------------ 1. one iteration at a time
def _case(name, p, l, k, D, reg="l1", alpha=None, seed=1):
    return pytest.param(dict(name=name, p=p, l=l, k=k, D=D, reg=reg, alpha=(1e-3 if reg == "l1" else 1e-4) if alpha is None else alpha,
                             seed=seed), id=name)


CASES = (
    [_case("p1-l1-k1", 1, 1, 1, "flat"), _case("p2-l2-k2", 2, 2, 2, "flat"), _case("p2-l2-k1", 2, 2, 1, "flat")]
    + [_case(f"p{p}-l5-k5", p, 5, 5, "flat") for p in (31, 32, 33, 127, 128, 129, 257)]
    + [_case(f"p300-l{l}-k{k}-{reg}", 300, l, k, "dec3", reg) for l, k in ((7, 1), (8, 4), (8, 8)) for reg in ("l1", "l0")]
    + [_case("p1000-l128-k30-lds", 1000, 128, 30, "dec3")]
    + [_case(f"p{p}-l128-k{k}-{reg}", p, 128, k, "dec6", reg) for p, k in ((129, 63), (4099, 64)) for reg in ("l1", "l0")]
    + [_case("p70000-l128-k64-partcap", 70000, 128, 64, "dec3"),      # G = min(547, 4 Mi / 8194 = 511) = 511
       _case("p262275-l2-k1-gmax", 262145 + 130, 2, 1, "flat"),       # G = SPCA_GMAX = 2048, 129 rows each, a remainder
       _case("p5000-l128-k64-tiny", 5000, 128, 64, "tiny"),
       _case("p300-l16-k4-zeroD", 300, 16, 4, "zero8")]
)


@pytest.mark.parametrize("case", CASES)
def test_one_step(ctx, case):
    V = make_V(case["p"], case["l"], case["seed"])
    D = spectrum(case["D"], case["l"], case["k"])
    Vd = dev(ctx, V)
    runs = {T: loop(ctx, Vd, D, case["k"], case["alpha"], 1e-3, case["reg"], max_iter=T) for T in (1, 2, 3)}
    for T, out in runs.items():
        assert out["n_iter"] == T
        assert np.all(np.isfinite(out["B"])) and np.all(out["objective"][T:] == SENT)
    figs, fails = check_steps(V, D, case["k"], case["alpha"], 1e-3, case["reg"], runs)
    print("\nSPCA-FIG" + figure_line(case["name"], figs))
    assert not fails, "\n".join(fails)
    if case["D"] == "tiny":         # two singular values of M lie below smax l eps: those columns took the completion branch
        assert all(np.all(runs[T]["dtilde"][case["k"] - 2:] <= case["l"] * EPS * runs[T]["dtilde"][0]) for T in runs)


def test_checker_rejects_a_wrong_rotation_and_a_wrong_partial():
    """CPU arithmetic only: the restated kernels pass check_steps, one wrong rotation angle / one wrong partial does not"""
    p, l, k, alpha, T = 300, 8, 4, 1e-3, 3
    V, D = make_V(p, l, 1), spectrum("dec3", l, k)
    clean = {t: emulate_loop(V, D, k, alpha, max_iter=t) for t in (1, 2, 3)}
    figs, fails = check_steps(V, D, k, alpha, 1e-3, "l1", clean)
    assert not fails, fails
    bad = dict(clean)
    bad[T] = emulate_loop(V, D, k, alpha, max_iter=T, wrong_rotation=(T, 1e-6))
    figs, fails = check_steps(V, D, k, alpha, 1e-3, "l1", bad)
    g, _, tol = figs[T]["polar"]["sym"]
    assert g > 1e3 * tol and any("polar sym" in f for f in fails), (g, tol, fails)
    bad[T] = emulate_loop(V, D, k, alpha, max_iter=T, wrong_partial=(T, 1e-6))
    figs, fails = check_steps(V, D, k, alpha, 1e-3, "l1", bad)
    d, tol = figs[T]["obj1"]
    assert d > 1e3 * tol and any("obj1" in f for f in fails) and any("obj2" in f for f in fails), (d, tol, fails)


# ------------------------------------------------------------------------------------------------ 2. zero columns
ZC = dict(p=4096, l=16, k=8, dense=(1, 3, 4, 6), rows=8, alpha=0.1)


def zero_column_V(seed=3):
    """V [p x l] orthonormal: the columns of `dense` (and k .. l - 1) dense with entries ~ 1 / sqrt(p), the other four of the
    first k supported on the first `rows` rows"""
    p, l, k, ns = ZC["p"], ZC["l"], ZC["k"], ZC["rows"]
    sparse = [c for c in range(k) if c not in ZC["dense"]]
    others = [c for c in range(l) if c not in sparse]
    X = np.random.default_rng(seed).standard_normal((p, l))
    X[ns:, :len(sparse)] = 0.0
    Q = np.linalg.qr(X, mode="reduced")[0]          # the sparse columns first: they stay on their rows
    V = np.empty((p, l))
    V[:, sparse], V[:, others] = Q[:, :len(sparse)], Q[:, len(sparse):]
    return V, sparse


def check_completion(V, D, Bprev, Qa, dt, n_dead):
    l, k = Qa.shape
    D2 = D * D
    M = np.asarray(D2[:, None] * hp_matmul(V.T, Bprev), np.float64)
    live = np.any(Bprev != 0.0, axis=0)
    assert (~live).sum() == n_dead and np.all(M[:, ~live] == 0.0)
    Us, s, Wt = np.linalg.svd(M[:, live], full_matrices=False)
    Ql = Us @ Wt
    assert np.abs(Qa[:, live] - Ql).max() <= 1e-9 * np.abs(Ql).max()          # the polar factor of the live columns
    Cc = Qa[:, ~live]
    assert np.abs(Cc.T @ Cc - np.eye(n_dead)).max() <= 1e-12
    assert np.abs(Us.T @ Cc).max() <= 1e-12                                   # orthogonal to the range of the live ones
    rule = completion_columns(list(Us.T), n_dead, l)                          # svd: descending singular values
    assert np.abs(Cc - rule).max() <= 1e-12, np.abs(Cc - rule).max()
    assert np.all(np.diff(dt) <= 0.0) and np.all(dt[live.sum():] == 0.0) and np.all(dt[:live.sum()] > 0.0)
    assert np.abs(dt[:live.sum()] - s).max() <= 1e-9 * s[0]
    return rule


def test_zero_columns_get_the_documented_completion(ctx):
    V, sparse = zero_column_V()
    D = spectrum("dec3", ZC["l"], ZC["k"])
    kappa = scaled(D, ZC["alpha"], 1e-3)[3]
    assert np.abs(V[:, list(ZC["dense"])]).max() < kappa < np.abs(V[:, sparse]).max(axis=0).min()
    Vd = dev(ctx, V)
    runs = {T: loop(ctx, Vd, D, ZC["k"], ZC["alpha"], max_iter=T) for T in (1, 2, 3)}
    for T in (1, 2, 3):
        zero = np.all(runs[T]["B"] == 0.0, axis=0)
        assert sorted(np.flatnonzero(zero)) == sorted(ZC["dense"]), (T, zero)            # zero from iteration 1 on, and stay so
    for T in (2, 3):
        rule = check_completion(V, D, runs[T - 1]["B"], runs[T]["Qa"], runs[T]["dtilde"], len(ZC["dense"]))
        # the live range leans on e_0, e_2, e_5, e_7 (the sparse columns of V), so the rule has to skip those unit vectors
        assert [int(np.argmax(np.abs(c))) for c in rule.T] == list(ZC["dense"])
        assert np.abs(rule - np.eye(ZC["l"])[:, list(ZC["dense"])]).max() > 1e-6         # ... and Gram-Schmidt did work
    figs, fails = check_steps(V, D, ZC["k"], ZC["alpha"], 1e-3, "l1", runs)              # update and objective hold as well
    assert not fails, "\n".join(fails)


def test_all_columns_zero(ctx):
    p, l, k = 300, 16, 4
    V, D = make_V(p, l, 5), spectrum("dec3", 16, 4)
    Vd = dev(ctx, V)
    for T in (2, 3):
        out = loop(ctx, Vd, D, k, alpha=10.0, max_iter=T)
        assert np.all(out["B"] == 0.0) and np.all(out["dtilde"] == 0.0)
        assert np.array_equal(out["Qa"], np.eye(l)[:, :k])                   # the first k unit vectors, exactly
        half = 0.5 * float((D.astype(LD) ** 2).sum())                        # 1/2 sum D^2 (|q|^2 + 1 - |q|^2)
        assert np.all(np.abs(out["objective"][:T] - half) <= l * U * 2.0 * half)


# ------------------------------------------------------------------------------------------------ 3. stopping, the batch of 16
FIXED = dict(p=300, l=8, k=4)


@pytest.fixture(scope="module")
def fixed_runs(ctx):
    V, D = make_V(FIXED["p"], FIXED["l"], 2), spectrum("dec3", FIXED["l"], FIXED["k"])
    Vd = dev(ctx, V)
    return {n: loop(ctx, Vd, D, FIXED["k"], max_iter=n) for n in (1, 2, 15, 16, 17, 32, 33)}


def test_fixed_counts_write_exactly_n_objectives_and_share_prefixes(fixed_runs):
    for n, out in fixed_runs.items():
        assert out["n_iter"] == n
        assert np.all(out["objective"][:n] != SENT) and np.all(np.isfinite(out["objective"][:n]))
        assert np.all(out["objective"][n:] == SENT) and out["objective"].size == n + 4
    longest = fixed_runs[33]["objective"]
    for n, out in fixed_runs.items():
        assert np.array_equal(out["objective"][:n], longest[:n]), n
    assert np.all(np.diff(longest[:33]) <= 1e-12 * longest[0])              # variable projection descends


def stop_design(tstar):
    """a problem whose reference objective sequence stops at iteration tstar for a tol that lies a factor >= 10 inside the
    gap between the decrement that must stop and every one before it.  Variable projection itself only slows down
    gradually, so the standstill is built: D = (1, 1e-3) and a first column of V of equal magnitudes (its column of B stays
    a multiple of it and settles at once), while the second column of B only loses kappa per iteration until its last
    entry dies -- from then on the objective stands still.  alpha places that at tstar."""
    p, l, k, n = 40, 2, 2, 40
    X = np.random.default_rng(4).standard_normal((p, l))
    X[:, 0] = np.sign(X[:, 0])
    V, D = np.linalg.qr(X, mode="reduced")[0], np.array([1.0, 1e-3])
    top = np.abs(V[:, 1]).max()
    alphas = [10.0] if tstar == 2 else np.linspace(top / (tstar + 2.0), top / max(tstar - 6.0, 1.0), 120)
    for alpha in alphas:
        o = emulate_loop(V, D, k, float(alpha), max_iter=n)["objective"]
        r = np.abs(o[:-1] - o[1:]) / o[1:]                                  # r[i - 1]: what iteration index i tests
        early = r[:tstar - 2]
        lo, hi = max(r[tstar - 2], 1e-14), (early.min() if early.size else 1.0)
        if hi >= 1e4 * lo:
            tol = float(np.sqrt(lo * hi))
            ref = emulate_loop(V, D, k, float(alpha), max_iter=n, tol=tol, check=1)
            assert ref["n_iter"] == tstar and r[tstar - 2] * 10.0 <= tol and np.all(early >= 10.0 * tol)
            return V, D, k, float(alpha), tol, n
    raise AssertionError(f"no alpha stops the reference at {tstar}")


@pytest.mark.parametrize("tstar", [2, 16, 17])
def test_stopped_run_equals_the_fixed_count_run(ctx, tstar):
    V, D, k, alpha, tol, n = stop_design(tstar)
    Vd = dev(ctx, V)
    stopped = loop(ctx, Vd, D, k, alpha, max_iter=n, tol=tol, check=1)
    assert stopped["n_iter"] == tstar
    assert np.all(stopped["objective"][tstar:] == SENT)
    fixed = loop(ctx, Vd, D, k, alpha, max_iter=tstar)
    assert same_state(stopped, fixed, tstar)                                # nothing enqueued after the stop touched the state
    if tstar == 2:                                                           # tol = 0 never stops, even at a standstill
        assert stopped["objective"][0] == stopped["objective"][1]
        never = loop(ctx, Vd, D, k, alpha, max_iter=20, tol=0.0, check=1)
        assert never["n_iter"] == 20 and np.all(never["objective"][:20] == stopped["objective"][0])


def test_null_objective_and_repeatability_at_the_limits(ctx):
    V, D = make_V(4099, 128, 7), spectrum("dec6", 128, 64)
    Vd = dev(ctx, V)
    a, b = loop(ctx, Vd, D, 64, max_iter=3), loop(ctx, Vd, D, 64, max_iter=3)
    assert same_state(a, b, 3)
    c = loop(ctx, Vd, D, 64, max_iter=3, want_obj=False)
    assert c["n_iter"] == 3 and c["objective"] is None
    assert np.array_equal(a["B"], c["B"]) and np.array_equal(a["Qa"], c["Qa"]) and np.array_equal(a["dtilde"], c["dtilde"])


# ------------------------------------------------------------------------------------------------ 4. the helper entries
def gram(ctx, X, a, Y, b, rows, ldx=None, ldy=None):
    """eofx_spca_gram_f64 on device tensors / views -> numpy [a x b]"""
    import torch

    from xeofs_amd._lib import ptr, raise_for

    out = torch.full((a, b), float("nan"), dtype=torch.float64, device=X.device)
    raise_for(ctx.lib.eofx_spca_gram_f64(ctx.handle, ptr(X), X.stride(0) if ldx is None else ldx, a, ptr(Y),
                                         Y.stride(0) if ldy is None else ldy, b, rows, ptr(out)), ctx.handle)
    return out.cpu().numpy()


def check_gram(got, X, Y, rows):
    ref = hp_matmul(X.T, Y)
    tol = rows * U * (np.abs(X).T @ np.abs(Y))
    err = np.abs(np.asarray(got.astype(LD) - ref, np.float64))
    assert np.all(err <= tol), (err / np.where(tol > 0, tol, 1.0)).max()


GRAM_AB = [(1, 1), (23, 89), (32, 64), (3, 683), (140, 64)]       # a b = 1, 2047, 2048, 2049 (one blockIdx.y holds 2048), 8960


@pytest.mark.parametrize("rows", [1, 127, 128, 129])
def test_gram_shapes_and_strided_views(ctx, rows):
    rng = np.random.default_rng(rows)
    for a, b in GRAM_AB:
        Xw, Yw = rng.standard_normal((rows, a + 5)), rng.standard_normal((rows, b + 9))
        Xd, Yd = dev(ctx, Xw)[:, 3:3 + a], dev(ctx, Yw)[:, 5:5 + b]         # column slices: row strides a + 5, b + 9
        assert Xd.stride(0) == a + 5 and Yd.stride(0) == b + 9
        got = gram(ctx, Xd, a, Yd, b, rows)
        check_gram(got, Xw[:, 3:3 + a], Yw[:, 5:5 + b], rows)
        assert np.array_equal(got, gram(ctx, Xd, a, Yd, b, rows))
        got = gram(ctx, Xd.contiguous(), a, Yd.contiguous(), b, rows)       # the same, stride = width
        check_gram(got, Xw[:, 3:3 + a], Yw[:, 5:5 + b], rows)


@pytest.mark.parametrize("a, b", [(1, 1), (32, 64)])
def test_gram_many_rows(ctx, a, b):
    rows = 300001                                                            # G = 2048: 147 rows each, the last one fewer
    rng = np.random.default_rng(a)
    X, Y = rng.standard_normal((rows, a)), rng.standard_normal((rows, b))
    Xd, Yd = dev(ctx, X), dev(ctx, Y)
    got = gram(ctx, Xd, a, Yd, b, rows)
    check_gram(got, X, Y, rows)
    assert np.array_equal(got, gram(ctx, Xd, a, Yd, b, rows))


@pytest.mark.parametrize("rows", [1, 129, 300001])
def test_gram_row_stride_zero(ctx, rows):
    rng = np.random.default_rng(rows)
    X = rng.standard_normal((rows, 6)) * 10.0 ** rng.uniform(-3, 3, (rows, 1))
    Xd = dev(ctx, X)
    ones, row = np.ones((1, 1)), rng.standard_normal((1, 7))
    got = gram(ctx, Xd, 6, dev(ctx, ones), 1, rows, ldy=0)                   # column sums
    check_gram(got, X, np.repeat(ones, rows, axis=0), rows)
    got = gram(ctx, Xd, 6, dev(ctx, row), 7, rows, ldy=0)                    # a general row, repeated
    check_gram(got, X, np.repeat(row, rows, axis=0), rows)


def test_sum_helper_over_twelve_decades(ctx):
    from xeofs_amd import spca

    n = 3_000_001
    rng = np.random.default_rng(12)
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 6.0, n)
    xd = dev1(ctx, x)
    tol = n * U * float(np.abs(x).sum(dtype=LD))
    s, sa = spca.spca_sum(ctx, xd), spca.spca_sum(ctx, xd, absolute=True)
    assert abs(float(s - x.sum(dtype=LD))) <= tol and abs(float(sa - np.abs(x).sum(dtype=LD))) <= tol
    assert s == spca.spca_sum(ctx, xd) and sa == spca.spca_sum(ctx, xd, absolute=True)


@pytest.mark.parametrize("a", [1, 128, 4096])
def test_rowmul_strided_views_leave_the_rest_untouched(ctx, a):
    import torch

    from xeofs_amd._lib import ptr, raise_for

    rng = np.random.default_rng(a)
    for b in (1, 64, 130):
        Mh = rng.standard_normal((a, b))
        Md = dev(ctx, Mh)
        for rows in (0, 1, 257):
            Xw = rng.standard_normal((max(rows, 1), a + 3))
            Xd = dev(ctx, Xw)[:, 2:2 + a]
            Yw = torch.full((max(rows, 1), b + 4), SENT, dtype=torch.float64, device=Xd.device)
            Yd = Yw[:, 1:1 + b]
            raise_for(ctx.lib.eofx_spca_rowmul_f64(ctx.handle, ptr(Xd), Xd.stride(0), a, ptr(Md), b, rows, ptr(Yd),
                                                   Yd.stride(0)), ctx.handle)
            Yh = Yw.cpu().numpy()
            assert np.all(Yh[:, :1] == SENT) and np.all(Yh[:, 1 + b:] == SENT)
            if rows == 0:
                assert np.all(Yh == SENT)
                continue
            X = Xw[:rows, 2:2 + a]
            err = np.abs(np.asarray(Yh[:rows, 1:1 + b].astype(LD) - hp_matmul(X, Mh), np.float64))
            assert np.all(err <= a * U * (np.abs(X) @ np.abs(Mh)))


def prox_dev(ctx, Xd, Yd, s, count, reg, kappa, out):
    from xeofs_amd._lib import ptr

    return ctx.lib.eofx_spca_prox_f64(ctx.handle, ptr(Xd), ptr(Yd), float(s), count, REG[reg], float(kappa), ptr(out))


def prox_inputs(count, kappa, edge):
    """X, Y of small dyadic rationals (X + s Y is exact for s = 1/2, fused or not), led by the edge values (with Y = 0)"""
    na, pa = np.nextafter, np.array
    edges = pa([edge, -edge, na(edge, 0.0), na(edge, 1.0), -na(edge, 0.0), -na(edge, 1.0), 0.0, -0.0])
    i = np.arange(count)
    X = ((i * 37) % 129 - 64) / 64.0
    Y = ((i * 11) % 65 - 32) / 32.0
    n = min(count, edges.size)
    X[:n], Y[:n] = edges[:n], 0.0
    if count > 20:                                                           # the edge reached as a sum: 1/2 + 1/2 * 1/2
        X[n:n + 2], Y[n:n + 2] = [edge - 0.25, -edge + 0.25], [0.5, -0.5]
    return X, Y


@pytest.mark.parametrize("reg", ["l1", "l0"])
@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_prox_is_exact_on_dyadic_inputs(ctx, reg, count):
    import torch

    from xeofs_amd._lib import raise_for

    edge = 0.75                                                              # |x| = kappa (l1 -> 0), x^2 = 2 kappa (l0 keeps x)
    for kappa in (edge if reg == "l1" else edge * edge / 2.0, 0.0):
        X, Y = prox_inputs(max(count, 1), kappa, edge)
        Xd, Yd = dev1(ctx, X), dev1(ctx, Y)
        out = torch.full((max(count, 1) + 3,), SENT, dtype=torch.float64, device=Xd.device)
        raise_for(prox_dev(ctx, Xd, Yd, 0.5, count, reg, kappa, out), ctx.handle)
        got = out.cpu().numpy()
        assert np.all(got[count:] == SENT)
        assert np.array_equal(got[:count], prox_np(X + 0.5 * Y, reg, kappa)[:count])
        out.fill_(SENT)
        raise_for(prox_dev(ctx, Xd, None, 0.5, count, reg, kappa, out), ctx.handle)       # Y = NULL: prox(X)
        assert np.array_equal(out.cpu().numpy()[:count], prox_np(X, reg, kappa)[:count])
        Xa = Xd.clone()
        raise_for(prox_dev(ctx, Xa, Yd, 0.5, count, reg, kappa, Xa), ctx.handle)          # out aliasing X
        assert np.array_equal(Xa.cpu().numpy()[:count], prox_np(X + 0.5 * Y, reg, kappa)[:count])
        assert np.array_equal(Xa.cpu().numpy()[count:], X[count:])
    if count == 257 and reg == "l1":                                         # what the edges must give, spelled out
        X, _ = prox_inputs(count, edge, edge)
        e = prox_np(X, "l1", edge)
        assert e[0] == 0.0 and e[1] == 0.0 and e[2] == 0.0 and e[3] == np.nextafter(edge, 1.0) - edge and e[5] == -e[3]
    if count == 257 and reg == "l0":
        X, _ = prox_inputs(count, edge * edge / 2.0, edge)
        e = prox_np(X, "l0", edge * edge / 2.0)
        assert e[0] == edge and e[1] == -edge and e[2] == 0.0 and e[3] == X[3] and e[4] == 0.0 and e[5] == X[5]


def test_rejections(ctx):
    import torch

    from xeofs_amd import _lib
    from xeofs_amd._lib import ptr

    def refused(rc, code):
        assert rc == code, (rc, code, last_error(ctx))
        assert last_error(ctx).strip()

    V = make_V(300, 129, 0)
    Vd, V128 = dev(ctx, V), dev(ctx, V[:, :128])
    D = np.logspace(0.0, -2.0, 129)
    # the loop
    refused(loop_raw(ctx, V[:, :8].copy(), D[:8], 4)[0], _lib.ERR_ARG)                    # a host pointer
    refused(loop_raw(ctx, V128, D[:128], 4, reg=2)[0], _lib.ERR_ARG)
    refused(loop_raw(ctx, dev(ctx, V[:, :4]), D[:4], 5)[0], _lib.ERR_ARG)                 # k > l
    refused(loop_raw(ctx, V128, D[:128], 65)[0], _lib.ERR_SHAPE)
    refused(loop_raw(ctx, Vd, D, 4)[0], _lib.ERR_SHAPE)                                   # l = 129
    for bad in ((0, np.nan), (3, np.nan), (0, 0.0), (5, -1.0), (2, np.inf)):
        Db = D[:128].copy()
        Db[bad[0]] = bad[1]
        refused(loop_raw(ctx, V128, Db, 4)[0], _lib.ERR_ARG)
    # gram
    X = dev(ctx, np.ones((4, 3)))
    out = torch.zeros((3, 3), dtype=torch.float64, device=X.device)
    g = ctx.lib.eofx_spca_gram_f64
    refused(g(ctx.handle, ptr(np.ones((4, 3))), 3, 3, ptr(X), 3, 3, 4, ptr(out)), _lib.ERR_ARG)
    refused(g(ctx.handle, ptr(X), 2, 3, ptr(X), 3, 3, 4, ptr(out)), _lib.ERR_ARG)          # ldx < a
    refused(g(ctx.handle, ptr(X), 3, 3, ptr(X), 2, 3, 4, ptr(out)), _lib.ERR_ARG)
    # rowmul
    r = ctx.lib.eofx_spca_rowmul_f64
    Xw, Mw = dev(ctx, np.ones((1, 4097))), dev(ctx, np.ones((4097, 1)))
    Y = torch.zeros((4, 3), dtype=torch.float64, device=X.device)
    refused(r(ctx.handle, ptr(Xw), 4097, 4097, ptr(Mw), 1, 1, ptr(Y), 3), _lib.ERR_ARG)   # a > 4096
    refused(r(ctx.handle, ptr(X), 2, 3, ptr(out), 3, 4, ptr(Y), 3), _lib.ERR_ARG)          # ldx < a
    refused(r(ctx.handle, ptr(X), 3, 3, ptr(out), 3, 4, ptr(Y), 2), _lib.ERR_ARG)          # ldy < b
    refused(r(ctx.handle, ptr(X), 3, 3, ptr(np.ones((3, 3))), 3, 4, ptr(Y), 3), _lib.ERR_ARG)
    assert np.all(Y.cpu().numpy() == 0.0)
    # prox
    x = dev1(ctx, np.ones(8))
    for kappa in (-1.0, np.nan, np.inf):
        refused(ctx.lib.eofx_spca_prox_f64(ctx.handle, ptr(x), None, 0.0, 8, 0, kappa, ptr(x)), _lib.ERR_ARG)
    refused(ctx.lib.eofx_spca_prox_f64(ctx.handle, ptr(x), None, 0.0, 8, 2, 0.5, ptr(x)), _lib.ERR_ARG)
    refused(ctx.lib.eofx_spca_prox_f64(ctx.handle, ptr(np.ones(8)), None, 0.0, 8, 0, 0.5, ptr(x)), _lib.ERR_ARG)
    assert np.all(x.cpu().numpy() == 1.0)


# ------------------------------------------------------------------------------------------------ 5. spca_svd, spca_orth
def _svd_matrix(kind):
    rng = np.random.default_rng(21)
    p, m = dict(tall=(40, 12), wide=(12, 40), square=(20, 20), deficient=(40, 12))[kind]
    Ct = rng.standard_normal((p, m)) * np.logspace(0.0, -2.0, m)
    if kind == "deficient":
        Ct[:, 7] = Ct[:, 3]                                                  # two equal columns: the Gram matrix is singular
    return Ct


@pytest.mark.parametrize("kind", ["tall", "wide", "square", "deficient"])
def test_spca_svd(ctx, kind, monkeypatch):
    import torch

    from xeofs_amd import spca

    calls = []
    qr = torch.linalg.qr
    monkeypatch.setattr(torch.linalg, "qr", lambda *a, **kw: (calls.append(1), qr(*a, **kw))[1])
    Ct = _svd_matrix(kind)
    p, m = Ct.shape
    V, D = spca.spca_svd(ctx, dev(ctx, Ct))
    V = V.cpu().numpy()
    assert len(calls) == (1 if kind == "deficient" else 0)                  # the Householder fallback, and only there
    r = min(p, m)
    assert V.shape == (p, r) and D.shape == (r,)
    assert np.abs(V.T @ V - np.eye(r)).max() <= 1e-12
    assert np.abs((V * D ** 2) @ V.T - Ct @ Ct.T).max() <= 1e-12 * D[0] ** 2
    assert np.all(np.diff(D) <= 0.0)
    assert np.abs(D - np.linalg.svd(Ct, compute_uv=False)).max() <= 1e-12 * D[0]
    assert np.all(V.max(axis=0) >= -V.min(axis=0))                          # signed: the largest-magnitude entry is positive
