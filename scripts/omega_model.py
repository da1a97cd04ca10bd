"""NumPy model of the edge recurrence of the Gram sequence.

The update pass of a step with a full window of three columns reads W_j, W_{j-1}, W_{j-2}; the read of W_{j-2} serves a
projection that is zero on well-behaved operators and measures the Gram entry W_{j+1} . W_{j-2}, which the next step needs
only to learn the same again. This model runs the step exactly as the device's finalize kernel assembles it (k_fin_gram:
unnormalised ring vectors W_t, nu_t = ||W_t||, every projection from Gram rows) and carries, beside every measured entry at
distance 3, the SIGNED estimate that the recurrence gives from entries at distances 1 and 2 - free-running: it is never fed a
measured distance-3 entry - together with the noise radius rho the device transports with it:

    D_j      = nu_t * sproj_j,      sproj_j = q_t . w  (t = j - 2) assembled with the distance-3 entry of row j
    rho_j    = (nu_t / nu_j) * rho_{j-1} + c * eps * ||A||_inf

Every dot is summed pairwise (np.sum over a contiguous axis): the nearest stand-in for the device's per-lane sums and partials
tree. With a sequentially summed dot the rounding of alpha alone puts |q_{j-2} . w| near the threshold on large grids.

    python scripts/omega_model.py            # the table of DESIGN.md §4.6
"""

from __future__ import annotations

import numpy as np
import scipy.sparse as sp

KAPPA = 4.0  # the certificate's bar is tol / KAPPA (slq.hip: kOmegaKappa)
C = 3.5  # a step adds C eps ||A||_inf to the radius (slq.hip: kOmegaC)


def laplacian(kind: str, m: int) -> sp.csr_matrix:
	T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
	I = sp.identity(m)
	if kind == "lap2d":
		return (sp.kron(I, T) + sp.kron(T, I)).tocsr()
	return (sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)).tocsr()


def _dot(X: np.ndarray, Y: np.ndarray) -> np.ndarray:
	"""Row-wise dots of two (P, n) C-ordered arrays, each summed pairwise."""
	return np.sum(X * Y, axis=1)


def run_model(A: sp.csr_matrix, k: int, nprobes: int, seed: int = 0, c: float = C) -> dict:
	"""Three-term Lanczos on `nprobes` Rademacher probes for k steps, assembled as the Gram sequence assembles it, with the
	free-running distance-3 estimate beside the measured entries. Returns maxima over steps and probes, in units of
	tol = 2 eps sqrt(n) unless named otherwise."""
	n = A.shape[0]
	eps = np.finfo(np.float64).eps
	tol = 2.0 * eps * np.sqrt(n)
	norm_inf = float(abs(A).sum(axis=1).max())
	theta = c * eps * norm_inf
	rng = np.random.default_rng(seed)
	P = nprobes
	W = {0: np.ascontiguousarray(rng.integers(0, 2, size=(P, n)) * 2.0 - 1.0)}
	nu = {0: np.sqrt(_dot(W[0], W[0]))}
	alpha = {}
	G = {}  # G[t][q] = W_t . W_{t-q}, measured
	g3_est = None  # the free-running estimate of G[j][3]
	rho = np.zeros(P)
	out = {"measured": 0.0, "est_err": 0.0, "est_err_over_rho": 0.0, "theta_needed_c": 0.0, "applied": 0, "steps": 0}
	for j in range(k):
		sc = 1.0 / nu[j]
		cp = nu[j] / nu[j - 1] if j > 0 else np.zeros(P)
		AW = np.ascontiguousarray((A @ W[j].T).T)
		a_raw = _dot(sc[:, None] * W[j], sc[:, None] * AW)  # q_j . (A q_j)
		a = a_raw - (sc * cp * G[j][1] if j > 0 else 0.0)
		alpha[j] = a
		cb = a / nu[j]
		w = sc[:, None] * AW - cb[:, None] * W[j]
		if j > 0:
			w -= cp[:, None] * W[j - 1]

		def sproj_of(i: int, hi) -> np.ndarray:  # k_fin_gram's expression for window position i (t = j - i)
			t = j - i
			s = G[j][i - 1] + (alpha[t] / nu[t]) * G[j][i]
			if t >= 1:
				s = s + (nu[t] / nu[t - 1]) * hi
			wt_wjm = nu[j - 1] ** 2 if i == 1 else G[j - 1][i - 1]
			d = sc * (nu[t] * s) - cp * wt_wjm
			return (d - cb * G[j][i]) / nu[t]

		r = min(j + 1, 3)
		gam = {}
		for i in range(1, r):
			sp_m = sproj_of(i, G[j].get(i + 1, np.zeros(P)))
			gam[i] = np.where(np.abs(sp_m) > tol, sp_m / nu[j - i], 0.0)
			if i == 2:
				out["measured"] = max(out["measured"], float(np.max(np.abs(sp_m))) / tol)
				if j >= 3:  # row j's distance-3 entry: measured against the free-running estimate
					sp_e = sproj_of(2, g3_est)
					rho = sc * nu[j - 2] * rho + theta
					err = np.abs(sp_e - sp_m)
					out["est_err"] = max(out["est_err"], float(np.max(err)) / tol)
					out["est_err_over_rho"] = max(out["est_err_over_rho"], float(np.max(err / rho)))
					# the one-step innovation: what theta has to cover, as c in c eps ||A||_inf
					innov = np.abs(G[j][3] - D_meas_prev) / nu[j - 3]
					out["theta_needed_c"] = max(out["theta_needed_c"], float(np.max(innov)) / (eps * norm_inf))
					out["steps"] += 1
				else:
					sp_e = sp_m
					rho = np.full(P, theta)
				g3_next = sp_e * nu[j - 2]  # W_{j+1} . W_{j-2} if the step applies no projection
				D_meas_prev = sp_m * nu[j - 2]
		for i, gm in gam.items():
			out["applied"] += int(np.count_nonzero(gm))
			w -= gm[:, None] * W[j - i]
		W[j + 1] = w
		G[j + 1] = {0: _dot(w, w)}
		for q in range(1, min(j + 2, 4)):
			G[j + 1][q] = _dot(w, W[j + 1 - q])
		nu[j + 1] = np.sqrt(G[j + 1][0])
		if r == 3:
			g3_est = g3_next
		W.pop(j - 2, None)
	out["rho_final_over_tol"] = float(np.max(rho)) / tol
	return out


CASES = [("lap2d", 1000, 30, 6), ("lap3d", 100, 30, 4), ("lap2d", 100, 100, 6), ("lap3d", 22, 300, 4)]


def main() -> None:
	print(f"{'case':<28}{'max |q_(j-2).w| / tol':>24}{'max |est - meas| / tol':>26}{'max |est - meas| / rho':>26}{'innovation, c':>16}")
	for kind, m, k, P in CASES:
		r = run_model(laplacian(kind, m), k, P)
		print(f"{kind + '_' + str(m) + ', k = ' + str(k) + ', ' + str(P) + ' probes':<28}{r['measured']:>24.4f}{r['est_err']:>26.4f}{r['est_err_over_rho']:>26.4f}{r['theta_needed_c']:>16.3f}")


if __name__ == "__main__":
	main()
