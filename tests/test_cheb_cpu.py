"""Chebyshev moments (the kernel polynomial method), the parts that need no device: the symbols, the launch decision
(`slq_debug_cheb_step_shape`), the host-side coefficients and damping factors, the NumPy yardstick of the GPU tests
(tests/_cheb_ref.py) against the exact eigen-formula, and the argument errors of the Python layer."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from _cheb_ref import grid_laplacian, moments_eig, moments_recurrence
from primate_amd import _capi

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ("slq_plan_create_chebyshev", "slq_plan_run_chebyshev", "slq_plan_get_moments", "slq_plan_moment_sum",
               "slq_density_update_moments", "slq_debug_cheb_step_shape")  # fmt: skip


def test_symbols_are_declared_exported_and_bound():
	hdr = (ROOT / "include" / "slq.h").read_text()
	L = _capi.lib()
	for s in NEW_SYMBOLS:
		assert re.search(rf"\bint {s}\(", hdr), f"{s} is not declared in slq.h"
		assert s in _capi.EXPORTED_SYMBOLS, f"{s} is not bound in _capi"
		assert hasattr(L, s), f"{s} is not exported by libslq"
	assert re.search(r"SLQ_DENSITY_CHEBYSHEV\s*=\s*4\b", hdr) and _capi.DENSITY_KINDS["chebyshev"] == 4
	assert re.search(r"constexpr int kMaxChebSteps = 16384;", (ROOT / "primate_amd" / "csrc" / "slq_format.hpp").read_text())
	from primate_amd import chebyshev, engine

	for name in ("run", "moments", "moment_sum", "describe", "set_probes", "set_probes_device", "generate_probes", "get_probes", "close"):
		assert callable(getattr(engine.ChebyshevPlan, name)), name
	for name in ("chebyshev_coefficients", "damping_factors", "spectral_bounds", "chebyshev_moments", "ChebyshevFunction"):
		assert hasattr(chebyshev, name), name


## ---- the launch decision -------------------------------------------------------------------------------------------
NF, NS, NC = 27, 18, 9
FACTS = ("csr", "far_le4", "tiles", "upper", "ringR", "rs_desc_u", "rs_u_padded", "deg", "orth", "nstale", "basis", "dense_class", "pipelined",
         "omega_on", "fused", "merged", "mgs", "stored_u", "nt", "cross", "gram", "gram_csr", "ring_gen", "ring_deep", "last_store", "ring_alpha",
         "ring_rev")  # fmt: skip
SHAPE = ("seq", "r", "tiled", "gen", "alpha_tiled", "alpha_upper", "half", "pipe_on", "xt_alpha", "xt_dots", "xt_update", "omega", "est_prev", "product",
         "blk_alpha", "blk_dots", "blk_beta", "prev_xt")  # fmt: skip
CHEB = ("sweeps", "tiled", "gen", "pipe_on", "xt_update", "product", "blk_product", "blk", "alpha_pass")
SEQ_SEPARATE, SEQ_SWEEPS_PLAIN = 3, 7
NSTEPS = 9


def facts_of(**kw):
	f = dict(csr=1, far_le4=1, tiles=0, upper=1, ringR=0, rs_desc_u=0, rs_u_padded=0, deg=NSTEPS, orth=3, nstale=0, basis=0, dense_class=0, pipelined=0,
	         omega_on=0, fused=1, merged=1, mgs=0, stored_u=1, nt=1, cross=1, gram=1, gram_csr=1, ring_gen=1, ring_deep=1, last_store=0, ring_alpha=2,
	         ring_rev=1)  # fmt: skip
	f.update(kw)
	return f


PLANS = {
	"ring-fed": facts_of(tiles=2, ringR=1, rs_desc_u=1, rs_u_padded=1),
	"ring-fed-narrow": facts_of(tiles=2, ringR=2, rs_desc_u=1, rs_u_padded=1),
	"barrier-tiles": facts_of(tiles=1, ringR=1),
	"generic": facts_of(),
	"generic-pipelined": facts_of(pipelined=1),
	"csr-sweeps": facts_of(far_le4=0),
	"csr-sweeps-ring-product": facts_of(far_le4=0, tiles=2, ringR=1),
	"dense": facts_of(csr=0, dense_class=4),
	"unfused": facts_of(csr=0, dense_class=0),
}
EXPECT_SWEEPS = {"csr-sweeps": 1, "csr-sweeps-ring-product": 1, "dense": 1, "unfused": 1}


def _shapes(f, j):
	L = _capi.lib()
	fa = (C.c_int * NF)(*[f[k] for k in FACTS])
	out_c = (C.c_int * NC)()
	assert L.slq_debug_cheb_step_shape(fa, NF, j, out_c, NC) == _capi.SLQ_OK
	f0 = dict(f, orth=0, nstale=0)
	fa0 = (C.c_int * NF)(*[f0[k] for k in FACTS])
	out_l = (C.c_int * (NS + 1))()
	assert L.slq_debug_step_shape(fa0, NF, j, 0, out_l, NS + 1) == _capi.SLQ_OK
	return dict(zip(CHEB, out_c[:])), dict(zip(SHAPE, out_l[:NS]))


@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("switches", [{}, {"cross": 0}, {"ring_rev": 0}, {"last_store": 1}, {"orth": 0}, {"orth": NSTEPS}], ids=str)
def test_cheb_step_takes_the_update_pass_of_the_orth0_lanczos_step(name, switches):
	f = dict(PLANS[name], **switches)
	for j in range(NSTEPS):
		c, l = _shapes(f, j)
		assert c["alpha_pass"] == 0
		assert c["xt_update"] & 1, "the cross term is a moment: always reduced"
		assert c["sweeps"] == EXPECT_SWEEPS.get(name, 0), (name, c)
		if c["sweeps"]:
			assert l["seq"] == SEQ_SWEEPS_PLAIN
			assert (c["product"], c["gen"], c["blk_product"]) == (l["product"], l["gen"], l["blk_alpha"])
			assert c["xt_update"] == 1 and c["blk"] == 1  # the streaming grid of k_cheb_axpy / k_cheb_3term, which always store
		else:
			assert l["seq"] == SEQ_SEPARATE and l["r"] == 0
			assert (c["tiled"], c["gen"], c["pipe_on"], c["blk"]) == (l["tiled"], l["gen"], l["pipe_on"], l["blk_beta"])
			assert c["xt_update"] == l["xt_update"] | 1
			assert (c["xt_update"] & ~(1 | 4 | 16)) == 0
		if c["xt_update"] & 16:
			assert j == NSTEPS - 1 and not switches.get("last_store"), "the no-store bit belongs to the last step"
	# where the Lanczos run may leave the last vector unstored, the Chebyshev run does: generic and k_ring_pass plans
	last, _ = _shapes(f, NSTEPS - 1)
	may = name in ("ring-fed", "ring-fed-narrow", "generic", "generic-pipelined") and not switches.get("last_store")
	assert bool(last["xt_update"] & 16) == may, (name, last)
	rev = name in ("ring-fed", "ring-fed-narrow") and switches.get("ring_rev", 1)
	assert bool(last["xt_update"] & 4) == bool(rev), (name, last)


def test_cheb_step_shape_rejects_wrong_sizes():
	L = _capi.lib()
	fa, out = (C.c_int * NF)(), (C.c_int * NC)()
	assert L.slq_debug_cheb_step_shape(fa, NF - 1, 0, out, NC) == _capi.SLQ_EINVAL
	assert L.slq_debug_cheb_step_shape(fa, NF, 0, out, NC + 1) == _capi.SLQ_EINVAL


## ---- host-side numerics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fun, f, bounds", [("exp", np.exp, (-1.0, 1.0)), ("exp", np.exp, (-2.0, 3.5)), ("log", np.log, (0.1, 8.0))])
def test_coefficients_match_chebinterpolate(fun, f, bounds):
	from numpy.polynomial import chebyshev as npc

	from primate_amd.chebyshev import chebyshev_coefficients

	a, b = bounds
	c, h = 0.5 * (a + b), 0.5 * (b - a)
	fmax = np.max(np.abs(f(c + h * np.cos(np.linspace(0, np.pi, 257)))))
	eps = np.finfo(float).eps
	for ncoef in (1, 2, 17, 64):
		# nquad = ncoef: the interpolant of chebinterpolate; the default (2 ncoef nodes): the head of the 2 ncoef-point interpolant.
		# Either way both sides are the same Chebyshev-Gauss sums of nquad terms of size <= max |f|: they differ by roundoff only
		for nquad in (ncoef, None):
			nq = ncoef if nquad is not None else 2 * ncoef
			ref = npc.chebinterpolate(lambda x: f(c + h * x), nq - 1)[:ncoef]
			for ff in (fun, f):  # the built-in name and the callable
				got = chebyshev_coefficients(ff, ncoef, bounds, nquad=nquad)
				assert got.shape == (ncoef,)
				assert np.max(np.abs(got - ref)) <= 8 * nq * eps * fmax, (fun, ncoef, nquad)


def test_damping_factors_closed_forms():
	from primate_amd.chebyshev import chebyshev_coefficients, damping_factors

	for N in (1, 2, 7, 64, 1001):
		k = np.arange(N)
		assert np.array_equal(damping_factors("none", N), np.ones(N)) and np.array_equal(damping_factors(None, N), np.ones(N))
		gj = damping_factors("jackson", N)
		ref = ((N - k + 1) * np.cos(np.pi * k / (N + 1)) + np.sin(np.pi * k / (N + 1)) / np.tan(np.pi / (N + 1))) / (N + 1)
		assert np.allclose(gj, ref, rtol=0, atol=4 * np.finfo(float).eps) and gj[0] == 1.0
		assert np.all(gj > 0) and np.all(np.diff(gj) < 0) if N > 1 else True
		gl = damping_factors("lanczos", N)
		ref = np.ones(N)
		ref[1:] = (np.sin(np.pi * k[1:] / N) / (np.pi * k[1:] / N)) ** 3
		assert np.allclose(gl, ref, rtol=0, atol=4 * np.finfo(float).eps) and gl[0] == 1.0
	c0 = chebyshev_coefficients("exp", 20, (-1, 1))
	assert np.allclose(chebyshev_coefficients("exp", 20, (-1, 1), damping="jackson"), c0 * damping_factors("jackson", 20), rtol=0, atol=0)


def test_spectral_bounds_gershgorin_contains_the_spectrum():
	from primate_amd.chebyshev import spectral_bounds

	A = grid_laplacian(9, 7)
	lam = np.linalg.eigvalsh(A.toarray())
	for M in (A, A.toarray(), (A + 0.3 * __import__("scipy.sparse").sparse.identity(63)).tocsr()):
		a, b = spectral_bounds(M)
		ev = np.linalg.eigvalsh(M.toarray() if hasattr(M, "toarray") else M)
		assert a <= ev[0] and ev[-1] <= b
	assert spectral_bounds(A) == (0.0, 8.0) and lam[0] > 0.0  # tight for a Laplacian
	a, b = spectral_bounds(np.eye(5) * 3.0)
	assert a < 3.0 < b


def test_reference_recurrence_matches_the_eigen_formula():
	"""The yardstick of the GPU tests, validated before the GPU meets it: 24^2 Laplacian, every k <= 400, bounds with and
	without slack. Bar: a step's rounding is at most g eps |w| with g = 8 (5 products and sums per row, the scalings and the
	three-term sum), it reaches mu_k through U_{k-i}(x), |U_m| <= m + 1, so |error_k| <= g eps mu_0 (k + 1)(k + 2) / 2 -
	a worst case over the spectrum; the dot itself adds log2(n) eps mu_0 (pairwise sums)."""
	m, K = 24, 401
	A = grid_laplacian(m, m)
	lam, U = np.linalg.eigh(A.toarray())
	rng = np.random.default_rng(5)
	Z = np.concatenate([np.sign(rng.standard_normal((m * m, 3))), rng.standard_normal((m * m, 2))], axis=1)
	eps = np.finfo(float).eps
	k = np.arange(K)
	for bounds in ((0.0, 8.0), (-0.5, 9.25)):
		ex = moments_eig(lam, U.T @ Z, K, bounds)
		got = moments_recurrence(A, Z, K, bounds)
		mu0 = np.sum(Z * Z, axis=0)
		assert np.allclose(ex[:, 0], mu0, rtol=1e-13)
		bar = (8.0 * (k + 1) * (k + 2) / 2 + 10.0) * eps * mu0[:, None]
		err = np.abs(got - ex)
		assert np.all(err <= bar), float(np.max(err / bar))
		assert np.all(np.abs(ex) <= mu0[:, None] * (1 + 1e-12))
	# the restatement carried in fp32 deviates at the fp32 scale and no more (what the GPU tests' bar is made of)
	g32 = moments_recurrence(A, Z, 40, (0.0, 8.0), dtype=np.float32)
	d = np.max(np.abs(g32 - moments_eig(lam, U.T @ Z, 40, (0.0, 8.0))), axis=1)
	assert np.all(d > 0) and np.all(d <= 8.0 * 41 * 42 / 2 * np.finfo(np.float32).eps * mu0)


## ---- argument errors of the Python layer, raised before any device work -------------------------------------------------
def test_argument_errors_before_any_device_work(monkeypatch):
	from primate_amd import chebyshev, engine, integrate

	def no_device(*a, **k):
		raise AssertionError("device work before the arguments were checked")

	monkeypatch.setattr(engine, "DeviceOperator", no_device)
	monkeypatch.setattr(engine, "default_context", no_device)
	monkeypatch.setattr(chebyshev, "_as_device_operator", no_device)
	A = grid_laplacian(6, 5)
	bad = [
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=0),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=True),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=40000),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=8, bounds=(1.0, 1.0)),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=8, bounds=(0.0, np.inf)),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=8, damping="fejer"),
		lambda: chebyshev.ChebyshevFunction(A, 3.0, deg=8),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=8, margin=0.0),
		lambda: chebyshev.ChebyshevFunction(A, "log", deg=8, bounds_method="power"),
		lambda: chebyshev.ChebyshevFunction(np.zeros((3, 4)), "log", deg=8),
		lambda: chebyshev.chebyshev_moments(A, deg=0),
		lambda: chebyshev.chebyshev_moments(A, deg=8, bounds=(2.0, 1.0)),
		lambda: chebyshev.chebyshev_moments(A, deg=8, nprobes=0),
		lambda: chebyshev.chebyshev_moments(A, deg=8, batch=0),
		lambda: chebyshev.chebyshev_moments(A, deg=8, pdf="cauchy"),
		lambda: chebyshev.chebyshev_moments(A, deg=8, pdf="device:cauchy"),
		lambda: chebyshev.chebyshev_coefficients("exp", 0, (-1, 1)),
		lambda: chebyshev.chebyshev_coefficients("exp", 8, (-1, 1), nquad=4),
		lambda: chebyshev.chebyshev_coefficients("exp", 8, (-1, 1), damping="fejer"),
		lambda: chebyshev.chebyshev_coefficients(np.log, 8, (-1, 1)),  # not finite on the bounds
		lambda: chebyshev.damping_factors("jackson", 0),
		lambda: chebyshev.spectral_bounds(A, method="power"),
		lambda: chebyshev.spectral_bounds(A, margin=-1.0),
		lambda: chebyshev.spectral_bounds(__import__("scipy.sparse.linalg").sparse.linalg.aslinearoperator(A), method="gershgorin"),
		lambda: integrate.spectral_density(A, method="kpm", kernel="lorentzian"),
		lambda: integrate.spectral_density(A, method="kpm", bw=0.1),
		lambda: integrate.spectral_density(A, method="kpm", bins=0),
		lambda: integrate.spectral_density(A, method="kpm", deg=0),
		lambda: integrate.spectral_density(A, method="kpm", damping="fejer"),
		lambda: integrate.spectral_density(A, method="kpm", interval=(3.0, 1.0)),
		lambda: integrate.spectral_density(A, method="kpm", pdf="cauchy"),
		lambda: integrate.spectral_density(A, method="chebyshev"),
	]
	for i, call in enumerate(bad):
		with np.errstate(all="ignore"), pytest.raises((ValueError, AssertionError)) as ei:
			call()
		assert "device work" not in str(ei.value), i
	assert integrate.DENSITY_KERNELS == ("gaussian", "lorentzian", "histogram", "cdf")
