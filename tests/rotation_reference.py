"""One step of the rotation loop (`eofx_panel_rot_step_f64`, include/eofx.h) in extended precision with a derived
componentwise error bound, and the cases tests/test_gpu_rot_step.py runs.  No GPU; tests/test_rotation_reference_cpu.py
checks this module on its own.

The step, for a float32 panel X [rows x L], R [L x L] float64, aux [L], per row b = x R:

  mode 0   t_j = b_j (b_j^2 - aux_j)                               G = X^T t
  mode 1   z = b_j / aux_j, t_j = z |z|^(power - 1)                G = b^T t
  mode 2   t_j = b_j (|b_j|^2 - aux_j)                             G = X^T t      |b_j|^2 = b_j^2 + b_{j +- L/2}^2: the panel is
  mode 3   t_j = (b_j / aux_j) (|b_j| / aux_j)^(power - 1)         G = b^T t      [Re | Im], R the real embedding (cpanel.embed)

`rot_step_ref` evaluates this in numpy's long double (unit roundoff 2^-64 on x86; the tests that need the headroom skip
where long double is float64).  `crot_step_ref` is the same step written in complex arithmetic, which shares no line with
the real embedding.

The bound B [L x L] is derived for a float64 evaluation, u = 2^-53, not tuned to any result:

  operands       db = (L + 2) u (|X| |R|)           a length-L inner product of exact float32 by float64 in any order
  transform      dt = |df/db| db + 4 u F(|b|, aux)  first order in db; F is the transform with absolute values everywhere
                                                    (mode 0: |b|^3 + |b| aux; mode 1: (|b| / aux)^power; ...), 4 u the roundings
                                                    of its few operations.  In modes 2 / 3 the partner part's db enters
                                                    through |b|^2 as well: + |dt_j/db_partner| db_partner.
  accumulation   B = (r + nbx + 2) u (|left|^T |t|) + |left|^T dt       r rows summed in any order, then the nbx partials
                 of the launcher (`eofx_panel_rot_step_f64`: one partial per workgroup, min(ceil(r / 32), 512 / 256 / 64))
  odd modes      + db^T |t|                         the left factor is b, not the exact x

The tests allow MARGIN * B + TINY.  The margin of 4 covers the second-order terms and the few ulp by which the device's
`pow`, `sqrt` and division may exceed one rounding each (nobody has measured them here); TINY = 2^-1000 only keeps 0 <= 0
true where the bound is exactly zero.  What the test is after -- a wrong partner column, a wrong left factor, a partial
left out or summed twice, a tile read at the wrong offset -- is an error of order 1 relative to |left|^T |t|, about
thirteen decimal orders above (r + nbx) u: the margin hides none of it.
The products inside B itself are float64 (relative error <= r u, far inside the margin).

Cases (`CASES`): every width, mode, column count and small row count crossed with every power; the row count just past
the point where a workgroup owns a second row tile once per width and mode; one set with the column scales spread over
1e-3 .. 1e3.  Data: unit-scale Gaussian rows (b takes both signs), a random orthogonal R (complex modes: a random
unitary one, embedded), two exactly zero rows whenever there are at least 31 (mode 3: |b| = 0; odd modes: pow(0, power - 1)).
"""

import functools

import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).eps < 2.0 ** -60
U = 2.0 ** -53
MARGIN = 4.0
TINY = 2.0 ** -1000

WG_CAP = {32: 512, 64: 512, 128: 256, 256: 64}        # workgroups of 32 rows the launchers start at most, by panel width
SMALL_ROWS = (1, 31, 32, 33)
POWERS = (1, 2, 3, 4)


def n_partials(rows, L):
    """partials the launcher sums: one per workgroup"""
    return max(1, min((rows + 31) // 32, WG_CAP[L]))


def rows_past_cap(L):
    """the smallest row count at which one workgroup owns two row tiles, plus one whole tile: 16416, 8224, 2080"""
    return (WG_CAP[L] + 1) * 32


def _partner(a, half):
    return np.roll(a, half, axis=1)


def rot_step_ref(X, R, aux, mode, power=1.0, nbx=1):
    """-> (G, B), both [L x L] long double: the step in extended precision and the float64 error bound of the docstring"""
    X, R, aux = np.asarray(X), np.asarray(R), np.asarray(aux)
    rows, L = X.shape
    half = L // 2
    if mode not in (0, 1, 2, 3) or R.shape != (L, L) or aux.shape != (L,) or (mode >= 2 and L % 2):
        raise ValueError("bad argument")
    q = LD(power) - 1
    Xl, ax = X.astype(LD), aux.astype(LD)
    b = Xl @ R.astype(LD)
    ab = np.abs(b)
    db = (L + 2) * U * (np.abs(X).astype(np.float64) @ np.abs(R).astype(np.float64)).astype(LD)
    dbp = None
    if mode == 0:
        t = b * (b * b - ax)
        d_own = np.abs(3 * b * b - ax)
        F = ab ** 3 + ab * np.abs(ax)
    elif mode == 1:
        z = b / ax
        zq = np.abs(z) ** q
        t = z * zq
        d_own = LD(power) * zq / np.abs(ax)
        F = np.abs(z) * zq
    else:
        bp = _partner(b, half)
        dbp = _partner(db, half)
        a2 = b * b + bp * bp
        if mode == 2:
            t = b * (a2 - ax)
            d_own = np.abs(a2 - ax + 2 * b * b)
            d_par = 2 * np.abs(b * bp)
            F = ab * (a2 + np.abs(ax))
        else:
            zq = (np.sqrt(a2) / ax) ** q                       # 0^0 = 1: a zero row gives t = b / aux = 0
            t = (b / ax) * zq
            pos = a2 > 0
            safe = np.where(pos, a2, LD(1))
            d_own = zq / np.abs(ax) * (1 + np.where(pos, q * b * b / safe, LD(0)))
            d_par = zq / np.abs(ax) * np.where(pos, q * np.abs(b * bp) / safe, LD(0))
            F = np.abs(t)
    dt = d_own * db + 4 * U * F
    if dbp is not None:
        dt = dt + d_par * dbp
    left = b if mode & 1 else Xl
    G = np.ascontiguousarray(left.T) @ t
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    la, ta = f64(np.abs(left)).T, f64(np.abs(t))
    B = (rows + nbx + 2) * U * (la @ ta) + la @ f64(dt)
    if mode & 1:
        B = B + f64(db).T @ ta
    return G, B.astype(LD)


def crot_step_ref(Z, Rc, auxh, mode, power=1.0):
    """the complex step in complex long double: Z [rows x m] complex, Rc [m x m], auxh [m] -> m x m
    mode 2: Z^H (b (|b|^2 - aux));  mode 3: b^H ((b / aux) (|b| / aux)^(power - 1)),  b = Z Rc"""
    CL = np.clongdouble
    Z, Rc, ax = np.asarray(Z).astype(CL), np.asarray(Rc).astype(CL), np.asarray(auxh).astype(LD)
    b = Z @ Rc
    a = np.abs(b)
    if mode == 2:
        return np.ascontiguousarray(Z.conj().T) @ (b * (a * a - ax))
    if mode == 3:
        return np.ascontiguousarray(b.conj().T) @ ((b / ax) * (a / ax) ** (LD(power) - 1))
    raise ValueError("bad argument")


def block_sum(B, m, half):
    """B [L x L] mapped through cpanel.block: the bounds of the real and of the imaginary part of the complex m x m block"""
    rr, ri = B[:m, :m], B[:m, half:half + m]
    ir, ii = B[half:half + m, :m], B[half:half + m, half:half + m]
    return rr + ii, ri + ir


def pack(Z, half):
    """complex [rows x m] -> float32 [Re | Im] panel of 2 half columns (cpanel.pack)"""
    r, m = Z.shape
    out = np.zeros((r, 2 * half), np.float32)
    out[:, :m], out[:, half:half + m] = Z.real, Z.imag
    return out


def unpack(X, m, half):
    return X[:, :m].astype(np.float64) + 1j * X[:, half:half + m].astype(np.float64)


def embed(Rc, half):
    """real embedding [[Rr, Ri], [-Ri, Rr]] of a complex m x m matrix in 2 half x 2 half (cpanel.embed)"""
    m = Rc.shape[0]
    E = np.zeros((2 * half, 2 * half))
    E[:m, :m] = E[half:half + m, half:half + m] = Rc.real
    E[:m, half:half + m] = Rc.imag
    E[half:half + m, :m] = -Rc.imag
    return E


# ----------------------------------------------------------------------------------------------------------------------
# cases: (L, mode, m, rows, power, spread); m counts real columns in modes 0 / 1 and complex ones in modes 2 / 3
def _widths(mode):
    return (32, 64, 128, 256) if mode < 2 else (64, 128, 256)


def _counts(L, mode):
    return (2, L - 1, L) if mode < 2 else (2, L // 2 - 1, L // 2)


def _cases():
    out = []
    for mode in range(4):
        powers = POWERS if mode & 1 else (1,)
        for L in _widths(mode):
            for m in _counts(L, mode):
                for rows in SMALL_ROWS:
                    out += [(L, mode, m, rows, pw, False) for pw in powers]
            out.append((L, mode, _counts(L, mode)[1], rows_past_cap(L), 3 if mode & 1 else 1, False))
        for L in (64, 256):
            out.append((L, mode, _counts(L, mode)[2], 33, 3 if mode & 1 else 1, True))
    return out


CASES = _cases()


def case_id(case):
    L, mode, m, rows, power, spread = case
    return f"L{L}-mode{mode}-m{m}-rows{rows}-pow{power}" + ("-spread" if spread else "")


@functools.lru_cache(maxsize=None)
def _operands(L, cplx, m, rows, spread):
    """X [rows x L] float32, R [L x L] float64 (+ the complex pair Z, Rc they embed), read-only"""
    rng = np.random.default_rng([L, int(cplx), m, rows, int(spread)])
    scale = 10.0 ** np.linspace(-3.0, 3.0, m) if spread else np.ones(m)
    half = L // 2
    if cplx:
        Z = (rng.standard_normal((rows, m)) + 1j * rng.standard_normal((rows, m))) * scale
        Rc = np.linalg.qr(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))[0]
        X, R = pack(Z, half), embed(Rc, half)
    else:
        X = np.zeros((rows, L), np.float32)
        X[:, :m] = rng.standard_normal((rows, m)) * scale
        R = np.zeros((L, L))
        R[:m, :m] = np.linalg.qr(rng.standard_normal((m, m)))[0]
        Rc = None
    if rows >= 31:
        X[[5, rows - 2]] = 0.0
    for a in (X, R):
        a.setflags(write=False)
    return X, R, Rc


def case_inputs(case):
    """-> dict X, R, aux (what the kernel takes) and, in the complex modes, Rc and auxh.  aux follows the loop: 0.7 of the
    column means of b^2 in the even modes (0.7: at one row the plain mean would cancel t to zero), the column maxima of |b| in
    the odd ones; padded with 0 / 1 as include/eofx.h requires"""
    L, mode, m, rows, power, spread = case
    cplx, half = mode >= 2, L // 2
    X, R, Rc = _operands(L, cplx, m, rows, spread)
    b = X.astype(np.float64) @ R
    a2 = b * b + (_partner(b * b, half) if cplx else 0.0)
    aux = np.ones(L) if mode & 1 else np.zeros(L)
    val = np.sqrt(a2).max(0) if mode & 1 else 0.7 * a2.mean(0)
    out = dict(X=X, R=R, mode=mode, power=float(power), nbx=n_partials(rows, L), m=m, half=half)
    if cplx:
        aux[:m] = aux[half:half + m] = val[:m]
        out.update(Rc=Rc, auxh=val[:m].copy())
    else:
        aux[:m] = val[:m]
    out["aux"] = aux
    return out


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """(G, B) of a case, computed once"""
    c = case_inputs(case)
    G, B = rot_step_ref(c["X"], c["R"], c["aux"], c["mode"], c["power"], c["nbx"])
    G.setflags(write=False)
    B.setflags(write=False)
    return G, B


def padding_mask(L, mode, m):
    """True where G must be an exact zero: rows and columns >= m (complex modes: >= m within each half)"""
    live = np.zeros(L, bool)
    live[:m] = True
    if mode >= 2:
        live[L // 2:L // 2 + m] = True
    return ~np.outer(live, live)
