"""Operators and run helpers of tests/test_gpu_omega.py (the edge recurrence of the Gram sequence)."""

import numpy as np
import scipy.sparse as sp

from conftest import laplacian_2d, laplacian_3d

OFF_KEYS = ("SLQ_OMEGA", "SLQ_OMEGA_TRIP", "SLQ_OMEGA_RESCUE")


def rademacher(n, P, seed, dtype=np.float64):
	rng = np.random.default_rng(seed)
	return np.asfortranarray(np.floor(rng.random((n, P)) * 2) * 2 - 1).astype(dtype)


def ill_conditioned(dtype=np.float64, m=100, decades=2.0):
	"""D L D with D spanning 10^-decades .. 10^decades on the 5-point pattern of an m x m grid (default: the ill-conditioned
	operator of tests/test_gpu_parity.py)."""
	rng = np.random.default_rng(99)
	L2 = laplacian_2d(m)
	dsc = 10.0 ** rng.uniform(-decades, decades, L2.shape[0])
	A = (sp.diags(dsc) @ L2 @ sp.diags(dsc)).tocsr()
	A.sort_indices()
	return A.astype(dtype)


def ragged_band(seed=31, dtype=np.float64, n=30011):
	"""A random symmetric band with gaps and a few empty off-diagonals, diagonally dominant (SPD): ragged workgroup tiles
	(tests/test_gpu_parity.py: the ragged case of the ring-fed passes)."""
	rng = np.random.default_rng(seed)
	offs = [1, 2, 150]
	D = [rng.uniform(0.2, 1.0, n - o) * (rng.random(n - o) > 0.15) for o in offs]
	B = sp.diags(D, offs, shape=(n, n))
	A = (B + B.T + sp.diags(np.full(n, 8.0))).tocsr()
	A.eliminate_zeros()
	A.sort_indices()
	return A.astype(dtype)


def fuzz_random_spd(n, deg, rng):
	"""scripts/fuzz_parity.py:random_spd: a weighted random graph Laplacian plus a random positive diagonal."""
	m = int(n * deg / 2)
	i, j = rng.integers(0, n, m), rng.integers(0, n, m)
	W = sp.coo_matrix((rng.uniform(0.1, 1.0, m), (i, j)), shape=(n, n)).tocsr()
	W = W + W.T
	A = (sp.diags(np.asarray(abs(W).sum(axis=1)).ravel() + rng.uniform(0.05, 1.0, n)) - W).tocsr()
	A.sort_indices()
	return A


def seed79():
	"""The seed-79 case of tests/test_gpu_parity.py (a short window that has lost orthogonality)."""
	rng = np.random.default_rng(79)
	n = int(rng.integers(1400, 1600))
	A = fuzz_random_spd(n, float(rng.uniform(1.0, 12.0)), rng)
	X = np.asfortranarray(np.floor(rng.random((n, 16)) * 2) * 2 - 1)
	return A, X


def run(eng, monkeypatch, op, X, deg, orth, env):
	"""One run of a fresh plan under `env` (the omega switches not named are unset): everything the tests compare."""
	for k in OFF_KEYS:
		monkeypatch.delenv(k, raising=False)
	for k, v in env.items():
		monkeypatch.setenv(k, str(v))
	plan = eng.LanczosPlan(op, X.shape[1], deg, orth)
	info = plan.describe()
	plan.set_probes(X)
	plan.run()
	alpha, beta, steps = plan.tridiag()
	out = {"info": info, "alpha": alpha, "beta": beta, "steps": steps, "log": plan.quadrature("log"), "exp": plan.quadrature("exp", t=-0.1),
	       "cols": plan.window_columns(), "verify": plan.window_verify(), "flags": plan.window_flags()}  # fmt: skip
	plan.close()
	for k in env:
		monkeypatch.delenv(k, raising=False)
	return out


__all__ = ["laplacian_2d", "laplacian_3d", "rademacher", "ill_conditioned", "ragged_band", "seed79", "run"]
