"""xeofs_amd.single.ArchetypalAnalysis -- archetypal analysis [Cutler & Breiman 1994, Technometrics 36, 338-347; Morup &
Hansen 2012, Neurocomputing 80, 54-63; in climate science: Hannachi & Trendafilov 2017, J. Climate 30, 6927-6944]: the field
is described by k EXTREME STATES, the archetypes.  Every archetype is a convex combination of observed samples and every
sample a convex combination of the archetypes.  Its modes are states one can point at (an El Nino, a La Nina, a blocked
flow), not sign-free patterns.  The reference has no such model; the definition is stated here in full.

With Xt [n x p] the engine's preprocessed float32 matrix of the fit (EOF._preprocess: masks, centring, standardising and
weights as in EOF),

    K   = Xt Xt^T  [n x n]                                   (ResidentMatrix.gram(0): float32, on the matrix cores)
    trK = sum_i K_ii                                         (float64)
    D_m = {x in R^m : x >= 0, sum x = 1}

find A [n x k] with rows in D_k and B [k x n] with rows in D_n that minimise

    f(A, B) = |Xt - A B Xt|_F^2 = trK - 2 <A, Q> + <S, M>,    Q = K B^T [n x k],  M = B Q [k x k],  S = A^T A [k x k].

The objective needs the field only through K: the field is read once for K and once for the archetype maps.  S, M, <.,.> and f
are float64 on the host from device results; the products with K are engine.panel_tmul (prec="f32") on engine.from_dense(K).

Algorithm
    1. start   idx = furthest_sum(K, k, start), start = RandomState(random_state).randint(n) -- the FurthestSum rule of Morup &
               Hansen on d(i, j)^2 = K_ii + K_jj - 2 K_ij: k - 1 greedy picks (the sample with the largest sum of distances to
               the picks so far), then one sweep that takes each pick out in turn and picks again; the lowest index wins
               ties; only the diagonal of K and the picked rows are read.  `init=` (k distinct sample indices) replaces it.
               B_0 = the one-hot rows of idx, A_0 = 1 / k.
    2. A step  L_A = lambda_max(M) (float64, host);  A <- simplex_pg(A, Q, M, 1 / L_A, iters)   (engine.simplex_pg: `iters`
               projected-gradient steps of every row in one launch), iters = init_iter in the first outer iteration and
               inner_iter afterwards.  1 / L_A is rounded to float32 towards zero.
    3. B step  G = (S B - A^T) K (one product with K);  trial B' = simplex_rows(B, G, mu) (engine.simplex_rows: the projection
               of every row of B - mu G onto D_n), Q' = K B'^T, M' = B' Q', f' from them.  Accept when f' <= f; then mu <- 2 mu
               while no trial has ever been rejected and mu <- 1.2 mu afterwards.  Otherwise mu <- mu / 2 and try again; after
               40 rejections in a row the fit stops with B unchanged and stats["stalled"] = True.
               mu_0 = 1 / (lambda_max(S) trK).  (The plain 1 / L step for B needs thousands of iterations on noisy fields.)
    4. stop    once a trial has been rejected at least once and f_prev - f' <= tol trK (f_prev: the f the outer iteration
               before ended with; f(A_0, B_0) for the first), or at max_iter.
    5. order   the modes by descending sum_i A_ik, the lowest index among equals.

    components()                    Z = B Xt as [p x k] in the input's coordinates and PREPROCESSED units (one
                                    engine.panel_tmul of B^T)
    archetypes()                    Z through the inverse preprocessing: the field's own units, the mean added back
    scores()                        A
    archetype_weights()             B as (mode, sample)
    explained_variance_fraction()   1 - f / trK
    objective_history()             f after every outer iteration
    transform(X')                   the fitted preprocessing, q = engine.project(X', Z), M = Z Z^T, then simplex_pg from 1 / k
                                    in batches of inner_iter iterations until a batch moves no entry by more than sqrt(tol),
                                    or 100 batches
    inverse_transform(scores)       engine.reconstruct(scores, Z) through the inverse preprocessing
    singular_values() and the other SVD-only accessors raise NotImplementedError

The model records per outer iteration the accepted mu (as the float32 the kernel was given), the inner count, the rejections
and f (stats["steps"]); tests/aa_reference.py replays them in float64.

Deliberate choices: the Gram form; the adaptive step; the order of the modes; components() in preprocessed
units against archetypes() in the field's own.  Out of scope: the sharded path, the bootstrapper, rotation, complex data, a
PCA pre-reduction.  Limits: n <= 16384 (K is 1 GB there and a row of B fills 64 KiB of LDS), k <= 32.

The host steps are module-level functions that need no GPU: check_modes, check_problem, furthest_sum, objective, mode_order,
step_down.
"""

from __future__ import annotations

import time

import numpy as np

from .. import engine, labelled
from .eof import EOF

N_MAX = engine.SIMPLEX_MMAX       # samples: a row of B is a row of simplex_rows
K_MAX = engine.SIMPLEX_KMAX       # modes: the variables of simplex_pg
MAX_REJECTIONS = 40
TRANSFORM_BATCHES = 100


def check_modes(n_modes) -> int:
    if not isinstance(n_modes, (int, np.integer)) or isinstance(n_modes, bool) or n_modes < 1:
        raise ValueError(f"ArchetypalAnalysis takes a positive integer n_modes, got {n_modes!r}")
    if n_modes > K_MAX:
        raise NotImplementedError(f"ArchetypalAnalysis takes at most {K_MAX} modes (the variables the projected-gradient kernel "
                                  f"holds in registers), got n_modes = {n_modes}")
    return int(n_modes)


def check_init(init, k: int):
    """None, or k distinct non-negative sample indices as an int64 array"""
    if init is None:
        return None
    idx = np.asarray(init)
    if idx.ndim != 1 or idx.size != k or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"init must hold n_modes = {k} integer sample indices, got {init!r}")
    idx = idx.astype(np.int64)
    if np.unique(idx).size != k:
        raise ValueError(f"init must hold distinct sample indices, got {idx.tolist()}")
    if idx.min() < 0:
        raise ValueError(f"init must hold sample indices >= 0, got {idx.tolist()}")
    return idx


def check_problem(n: int, k: int, init=None):
    """the refusals that need the number of samples"""
    if k > n:
        raise ValueError(f"n_modes must be at most the number of samples: n_modes = {k}, n_samples = {n}")
    if n > N_MAX:
        raise NotImplementedError(f"ArchetypalAnalysis takes at most {N_MAX} samples (the Gram matrix is 1 GB there and a row of the "
                                  f"archetype weights fills 64 KiB of LDS), got n_samples = {n}")
    if init is not None and np.max(init) >= n:
        raise ValueError(f"init names sample {int(np.max(init))}, the field has n_samples = {n}")


def _rows_of(K):
    """(diagonal, row(i)) of a symmetric matrix as float64 host arrays: a numpy array or a device tensor, of which only the
    diagonal and the rows asked for are fetched"""
    if hasattr(K, "data_ptr"):
        return (K.diagonal().detach().cpu().numpy().astype(np.float64),
                lambda i: K[int(i)].detach().cpu().numpy().astype(np.float64))
    K = np.asarray(K)
    return np.diagonal(K).astype(np.float64), lambda i: K[int(i)].astype(np.float64)


def furthest_sum(K, k: int, start: int) -> np.ndarray:
    """The FurthestSum rule (Morup & Hansen 2012, section 2.2) on d(i, j) = sqrt(max(K_ii + K_jj - 2 K_ij, 0)), float64:
    picks = [start]; k - 1 times the sample outside the picks with the largest sum of distances to the picks; then, for k >= 2,
    one sweep t = 0 .. k - 1 that takes pick t out and puts in its place the sample outside the others with the largest sum of
    distances to the others.  The lowest index wins ties.  -> k distinct indices (int64)."""
    diag, row = _rows_of(K)
    n = diag.size

    def dist(i):
        return np.sqrt(np.maximum(diag[i] + diag - 2.0 * row(i), 0.0))

    def pick(total, taken):
        t = np.where(taken, -np.inf, total)
        return int(np.argmax(t))                   # (argmax: the first of equals)

    picks = [int(start)]
    d = {picks[0]: dist(picks[0])}
    total = d[picks[0]].copy()
    taken = np.zeros(n, dtype=bool)
    taken[picks[0]] = True
    for _ in range(k - 1):
        j = pick(total, taken)
        picks.append(j)
        taken[j] = True
        d[j] = dist(j)
        total += d[j]
    if k >= 2:
        for t in range(k):
            old = picks[t]
            total -= d.pop(old)
            taken[old] = False
            j = pick(total, taken)
            picks[t] = j
            taken[j] = True
            d[j] = dist(j)
            total += d[j]
    return np.asarray(picks, dtype=np.int64)


def objective(trK: float, A, Q, S, M) -> float:
    """f = trK - 2 <A, Q> + <S, M> in float64"""
    return float(trK - 2.0 * np.sum(np.asarray(A, np.float64) * np.asarray(Q, np.float64)) + np.sum(S * M))


def mode_order(A) -> np.ndarray:
    """the modes by descending sum_i A_ik, the lowest index among equals"""
    return np.argsort(-np.asarray(A, dtype=np.float64).sum(axis=0), kind="stable")


def step_down(x: float) -> np.float32:
    """x > 0 as a float32 that does not exceed it"""
    y = np.float32(x)
    return np.nextafter(y, np.float32(0)) if float(y) > x else y


def _lambda_max(M) -> float:
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.eigvalsh(0.5 * (M + M.T))[-1])


def _svd_only(what: str):
    def accessor(self, *args, **kwargs):
        raise NotImplementedError(f"ArchetypalAnalysis has no {what}: archetypes are not singular vectors, "
                                  "explained_variance_fraction() gives the share of the variance the fit holds")

    return accessor


class ArchetypalAnalysis(EOF):
    """Archetypal analysis.  archetypes() are the extreme states in the field's units, components() the same in preprocessed
    units, scores() the convex weights A of every sample, archetype_weights() the convex weights B that build the archetypes
    from the samples."""

    def __init__(self, n_modes: int = 2, center: bool = True, standardize: bool = False, use_coslat: bool = False,
                 check_nans=True, sample_name: str = "sample", feature_name: str = "feature",
                 random_state: int | None = None, max_iter: int = 500, tol: float = 1e-6, inner_iter: int = 10,
                 init_iter: int = 50, init=None):
        k = check_modes(n_modes)
        if not isinstance(tol, (int, float, np.integer, np.floating)) or not tol >= 0.0:
            raise ValueError(f"tol must be >= 0, got {tol!r}")
        for name, v in (("max_iter", max_iter), ("inner_iter", inner_iter), ("init_iter", init_iter)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        init = check_init(init, k)
        super().__init__(n_modes=k, center=center, standardize=standardize, use_coslat=use_coslat, check_nans=check_nans,
                         sample_name=sample_name, feature_name=feature_name, compute=True, random_state=random_state)
        own = dict(max_iter=int(max_iter), tol=float(tol), inner_iter=int(inner_iter), init_iter=int(init_iter))
        self.attrs.update({"model": "Archetypal analysis", **own, "init": "None" if init is None else str(init.tolist())})
        self._params.update({**own, "init": init})

    # ------------------------------------------------------------------ fit
    def _fit_now(self, X, dim, weights=None):
        if labelled.is_complex(X):
            raise TypeError("This method does not support complex data.")
        mat = self._preprocess(X, dim, weights)
        try:
            return self._fit_algorithm(mat)
        except BaseException:
            mat.free()
            raise

    def _fit_algorithm(self, mat, omega=None, dec=None):
        """the module's algorithm on the resident preprocessed field `mat`"""
        torch = engine._torch()
        ctx, prm = self.ctx, self._params
        n, p = mat.shape
        k, init = int(self.n_modes), prm["init"]
        check_problem(n, k, init)
        ms = dict(gram=0.0, kprod=0.0, simplex_pg=0.0, simplex_rows=0.0, host=0.0)
        tick = time.perf_counter
        t_all = tick()

        def timed(name, fn, *args, **kwargs):
            t0 = tick()
            out = fn(*args, **kwargs)
            ctx.synchronize()
            ms[name] += 1e3 * (tick() - t0)
            return out

        Kd = timed("gram", lambda: mat.gram(0)[:n, :n].contiguous())
        diag = Kd.diagonal().cpu().numpy().astype(np.float64)
        trK = float(diag.sum())
        if not trK > 0.0:
            raise ValueError("ArchetypalAnalysis needs a field with variance: the preprocessed field is zero")
        Kmat = engine.from_dense(ctx, Kd)
        L = engine.panel_width(k)
        Zn = torch.zeros((Kmat.n_pad, L), dtype=torch.float32, device=Kd.device)
        products = [0]

        def kprod(W):
            """K W for W [n x k] (a device tensor or a host array) -> a device view [n x k] of a new panel"""
            Zn[:n, :k] = W if hasattr(W, "data_ptr") else torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).to(Zn.device)
            products[0] += 1
            return timed("kprod", engine.panel_tmul, ctx, Kmat, Zn, prec="f32")[:n, :k]

        def host(t):
            return t.cpu().numpy().astype(np.float64)

        try:
            if init is None:
                start = int(np.random.RandomState(prm["random_state"]).randint(n))
                idx = furthest_sum(Kd, k, start)
            else:
                start, idx = None, init
            Bd = torch.zeros((k, n), dtype=torch.float32, device=Kd.device)
            Bd[torch.arange(k, device=Kd.device), torch.as_tensor(idx, device=Kd.device)] = 1.0
            Ad = torch.full((n, k), 1.0 / k, dtype=torch.float32, device=Kd.device)
            Qd = kprod(Bd.t())
            Bh, Q, Ah = host(Bd), host(Qd), host(Ad)
            M, S = Bh @ Q, Ah.T @ Ah
            f = f_start = objective(trK, Ah, Q, S, M)
            mu = 1.0 / (_lambda_max(S) * trK)
            rejected_ever = stalled = False
            history, steps = [], []
            for it in range(prm["max_iter"]):
                iters = prm["init_iter"] if it == 0 else prm["inner_iter"]
                inv_L = step_down(1.0 / max(_lambda_max(M), np.finfo(np.float64).tiny))
                timed("simplex_pg", engine.simplex_pg, ctx, Ad, Qd, M, inv_L, iters, out=Ad)
                Ah = host(Ad)
                S = Ah.T @ Ah
                fA = objective(trK, Ah, Q, S, M)
                G = kprod((S @ Bh - Ah.T).T).t().contiguous()
                rej = 0
                while True:
                    mu32 = np.float32(mu)
                    Bn = timed("simplex_rows", engine.simplex_rows, ctx, Bd, G, mu32)
                    Qn_d = kprod(Bn.t())
                    Bn_h, Qn = host(Bn), host(Qn_d)
                    Mn = Bn_h @ Qn
                    fn = objective(trK, Ah, Qn, S, Mn)
                    if fn <= fA:
                        Bd, Qd, Bh, Q, M = Bn, Qn_d, Bn_h, Qn, Mn
                        mu *= 1.2 if rejected_ever else 2.0
                        break
                    rejected_ever = True
                    rej += 1
                    mu /= 2.0
                    if rej == MAX_REJECTIONS:
                        stalled, fn = True, fA
                        break
                steps.append(dict(mu=float(mu32), inner=int(iters), rejections=rej, f=fn, accepted=not stalled))
                history.append(fn)
                f_prev, f = f, fn
                if stalled or (rejected_ever and f_prev - f <= prm["tol"] * trK):
                    break
            order = mode_order(Ah)
            Ah, Bh = Ah[:, order], Bh[order]
            Bp = engine.panel_import(ctx, np.ascontiguousarray(Bh.T, dtype=np.float32), mat.n_pad, L)
            Z = mat.compact_rows(engine.panel_export(ctx, engine.panel_tmul(ctx, mat, Bp, prec="f32"), mat.p_phys, k))
        finally:
            Kmat.free()
        total = 1e3 * (tick() - t_all)
        ms["host"] = total - sum(v for name, v in ms.items() if name != "host")
        self.data = dict(input_data=mat, components=np.ascontiguousarray(Z, dtype=np.float32), scores=Ah.astype(np.float32),
                         weights=Bh.astype(np.float32), objective=f, trK=trK, history=np.asarray(history, dtype=np.float64),
                         mode_order=order)
        self.stats = dict({f"ms_{name}": v for name, v in ms.items()}, ms_total=total, iterations=len(history),
                          products=products[0], stalled=stalled, start=start, init_index=np.asarray(idx, dtype=np.int64),
                          f_start=f_start, steps=steps)
        return self

    # ------------------------------------------------------------------ transform / inverse
    def transform(self, X):
        """new data -> the fitted preprocessing -> q = X' Z -> simplex_pg from 1 / k in batches of inner_iter iterations, until a
        batch moves no entry by more than sqrt(tol) (or 100 batches)"""
        self.compute()
        torch = engine._torch()
        ctx, prm = self.ctx, self._params
        Z = self.data["components"]
        mat, fields, vs = self.preprocessor.transform(X)
        try:
            q = engine.project(ctx, mat, Z)
        finally:
            mat.free()
        Z64 = Z.astype(np.float64)
        M = Z64.T @ Z64
        inv_L = step_down(1.0 / max(_lambda_max(M), np.finfo(np.float64).tiny))
        k = Z.shape[1]
        dev = f"cuda:{ctx.device}"
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
        a = torch.full(tuple(qd.shape), 1.0 / k, dtype=torch.float32, device=dev)
        batches = 0
        for batches in range(1, TRANSFORM_BATCHES + 1):
            new = engine.simplex_pg(ctx, a, qd, M, inv_L, prm["inner_iter"])
            moved = float((new - a).abs().max()) if new.numel() else 0.0
            a = new
            if not moved > np.sqrt(prm["tol"]):      # (a NaN row stops nothing: it never changes again)
                break
        self.stats = dict(getattr(self, "stats", {}), transform_batches=batches)
        return self.preprocessor.inverse_transform_scores(a.cpu().numpy(), "scores", self.attrs, fields, vs)

    def inverse_transform(self, scores):
        """scores [.., mode] -> engine.reconstruct(scores, Z) through the inverse preprocessing"""
        self.compute()
        S, modes, vs, fields = self._parse_scores(scores, False, np.float32)
        Z = np.ascontiguousarray(self.data["components"][:, modes - 1])
        return self.preprocessor.inverse_transform_data(engine.reconstruct(self.ctx, S, Z), "reconstructed_data", fields, vs)

    # ------------------------------------------------------------------ accessors
    def components(self):
        """Z = B Xt: the archetypes in preprocessed units, as (mode, features)"""
        return self.preprocessor.inverse_transform_components(self.data["components"], "components", self.attrs)

    def archetypes(self):
        """the archetypes in the field's own units: Z through the inverse preprocessing (weights, deviation, mean)"""
        pre = self.preprocessor
        vf = pre.valid_feature
        Z = self.data["components"].astype(np.float64).T          # [k x p]
        if pre.feature_weights is not None:
            Z = Z / pre.feature_weights[vf]
        if pre.std_ is not None:
            Z = Z * pre.std_[vf]
        if pre.mean_ is not None:
            Z = Z + pre.mean_[vf]
        return pre.inverse_transform_components(np.ascontiguousarray(Z.T), "archetypes", self.attrs)

    def scores(self):
        """A: the convex weights of the archetypes in every sample"""
        return self.preprocessor.inverse_transform_scores(self.data["scores"], "scores", self.attrs)

    def archetype_weights(self):
        """B as (mode, sample): the convex weights of the samples in every archetype"""
        return self.preprocessor.inverse_transform_scores(np.ascontiguousarray(self.data["weights"].T), "archetype_weights",
                                                          self.attrs)

    def explained_variance_fraction(self) -> float:
        """1 - f / trK"""
        self.compute()
        return 1.0 - self.data["objective"] / self.data["trK"]

    def objective_history(self) -> np.ndarray:
        """f after every outer iteration"""
        self.compute()
        return self.data["history"].copy()

    singular_values = _svd_only("singular values")
    explained_variance = _svd_only("explained variance per mode")
    explained_variance_ratio = _svd_only("explained variance ratio per mode")
