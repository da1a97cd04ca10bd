"""Gauss quadrature from a Jacobi matrix — same signature as the reference's
`primate.integrate.quadrature` (src/primate/integrate.py:9-76); the eigen-solve runs in libslq's
on-device implicit-QL kernel instead of LAPACK stemr (src/primate/tridiag.py:10-11).
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from . import engine


def quadrature(
	d: np.ndarray,
	e: np.ndarray,
	deg: Optional[int] = None,
	quad: str = "gw",
	nodes: Optional[np.ndarray] = None,
	weights: Optional[np.ndarray] = None,
	endpoint: Optional[float] = None,
	residual: Optional[float] = None,
	**kwargs,
) -> tuple:
	"""Nodes (ascending eigenvalues of T(d, e)) and weights (squared first eigenvector components)
	of the degree-`deg` Gauss rule. `e` may have len(d) entries (e[0] = 0) or len(d) - 1.
	quad="radau": the (deg + 1)-point Gauss-Radau rule with a prescribed node at `endpoint` (a lower bound of the
	spectrum); `residual` is beta_deg, the coupling of T to its border (the norm of the Lanczos residual after deg steps)."""
	if quad == "radau":  # (checked before any device work)
		if endpoint is None or not np.isfinite(float(endpoint)):
			raise ValueError("quad='radau' needs a finite endpoint=a with a <= lambda_min")
		if residual is None or not np.isfinite(float(residual)):
			raise ValueError("quad='radau' needs residual=beta_deg, the norm of the Lanczos residual after deg steps")
	elif endpoint is not None or residual is not None:
		raise ValueError("endpoint and residual belong to quad='radau'")
	d = np.asarray(d)
	e = np.asarray(e)
	deg = len(d) if deg is None else int(min(deg, len(d)))
	e = np.append([0], e) if len(e) == (len(d) - 1) else e
	assert len(d) == len(e) and np.isclose(e[0], 0.0), "Subdiagonal first element 'e[0]' must be close to zero"
	if quad in {"gw", "golub_welsch"}:
		theta, tau = engine.quadrature_batch(d[:deg][None, :], e[:deg][None, :])
		theta, tau = theta[0].astype(d.dtype, copy=False), tau[0].astype(d.dtype, copy=False)
	elif quad == "fttr":
		## nodes of the FULL Jacobi matrix, weights by the forward three-term recurrence over all of
		## (d, e) for the first `deg` nodes (integrate.py:65-69, fttr.py:17-29), both on the device
		theta, _ = engine.quadrature_batch(d[None, :], e[None, :])
		theta = theta[0].astype(d.dtype, copy=False)
		tau = np.zeros(len(theta), dtype=theta.dtype)
		tau[:deg] = engine.fttr_batch(theta[None, :], d[None, :], e[None, :], k=deg)[0]
	elif quad == "radau":
		theta, tau = engine.quadrature_radau_batch(d[:deg][None, :], e[:deg][None, :], [float(residual)], float(endpoint))
		theta, tau = theta[0].astype(d.dtype, copy=False), tau[0].astype(d.dtype, copy=False)
	else:
		raise ValueError(f"Invalid quadrature method '{quad}' supplied")
	if nodes is not None and weights is not None:
		assert len(nodes) == len(theta) and len(weights) == len(theta), "`nodes` and `weights` output arrays must be `deg` in length (deg + 1 for quad='radau')."
		np.copyto(nodes, theta)
		np.copyto(weights, tau)
	return theta, tau


## ---------------------------------------------------------------------------------------------------------------------
## spectral density (the reference plans it: `from .integrate import spectral_density`, src/primate/__init__.py:10)
## ---------------------------------------------------------------------------------------------------------------------
DENSITY_KERNELS = ("gaussian", "lorentzian", "histogram", "cdf")
## interval=None: the hull of the first batch's nodes, widened by this fraction of its width on each side
INTERVAL_MARGIN = 0.1


def _density_args(kernel, bins, interval, bw, nprobes, batch, pdf) -> tuple:
	"""Checks every argument of `spectral_density` before any device work; returns (bins, interval, bw)."""
	if kernel not in DENSITY_KERNELS:
		raise ValueError(f"unknown kernel '{kernel}' (one of {', '.join(DENSITY_KERNELS)})")
	if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
		raise ValueError(f"bins must be an integer >= 1, got {bins!r}")
	if interval is not None:
		a, b = (float(v) for v in interval)
		if not (np.isfinite(a) and np.isfinite(b) and a < b):
			raise ValueError(f"interval must be finite with a < b, got {interval!r}")
		interval = (a, b)
	if bw is not None:
		bw = float(bw)
		if not (np.isfinite(bw) and bw > 0.0):
			raise ValueError(f"bw must be > 0, got {bw!r}")
	for name, v in (("nprobes", nprobes), ("batch", batch)):
		if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
			raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
	from ._capi import PDF_IDS
	from .random import _ISO_DISTRIBUTIONS

	if not isinstance(pdf, str):
		raise ValueError("pdf must be a distribution name or 'device:<name>'")
	name = pdf[len("device:"):] if pdf.startswith("device:") else pdf
	if name not in (PDF_IDS if pdf.startswith("device:") else _ISO_DISTRIBUTIONS):
		raise ValueError(f"Invalid distribution '{pdf}' supplied.")
	return int(bins), interval, bw


def _density_grid(kernel: str, bins: int, a: float, b: float) -> np.ndarray:
	return np.linspace(a, b, bins + 1 if kernel == "histogram" else bins)


def _density_accumulate(M, kernel, bins, interval, bw, lo: int, hi: int, batch: int, pdf: str, seed):
	"""Probe ids [lo, hi) of the stream (pdf, seed) through lock-step runs of `batch` probes, folded on the device.
	Host draws replay the `isotropic` stream of `hutch` (columns lo.. of default_rng(seed)); "device:<name>" draws
	Philox probe ids lo, lo + 1, ... Returns (mean, M2, outside, count, grid, interval, bw)."""
	from .engine import DensityAccumulator, LanczosPlan
	from .random import isotropic

	op, deg, orth, rtol = M._op, M._deg, M._orth, M._rtol
	n = op.shape[0]
	rng = np.random.default_rng(seed)
	dev_pdf = pdf[len("device:"):] if pdf.startswith("device:") else None
	if dev_pdf is not None:
		dev_seed = int(seed) if isinstance(seed, (int, np.integer)) else int(rng.integers(0, 2**62))
	else:
		draw = isotropic(pdf=pdf, seed=rng)
		for s0 in range(0, lo, batch):  # (column-major draws: the stream's first lo columns, skipped a batch at a time)
			draw(size=(n, min(batch, lo - s0)))
	plans, acc, grid = {}, None, None
	try:
		done = lo
		while done < hi:
			m = min(batch, hi - done)
			if m not in plans:
				plans[m] = LanczosPlan(op, m, deg, orth)
			plan = plans[m]
			if dev_pdf is not None:
				plan.generate_probes(dev_pdf, seed=dev_seed, probe_offset=done)
			else:
				plan.set_probes(draw(size=(n, m)).astype(op.dtype, copy=False))
			plan.run(rtol)
			if acc is None:
				if interval is None:
					## the hull of the first batch's nodes (zero-weight nodes of an early stop excluded); its QL is the one the
					## accumulator's update then reuses
					_, nodes, weights = plan.quadrature("identity", return_rule=True)
					th = nodes[weights > 0]
					t0, t1 = (float(th.min()), float(th.max())) if th.size else (0.0, 0.0)
					w = (t1 - t0) if t1 > t0 else max(abs(t1), 1.0)
					interval = (t0 - INTERVAL_MARGIN * w, t1 + INTERVAL_MARGIN * w)
				if bw is None:
					bw = (interval[1] - interval[0]) / plan.deg
				grid = _density_grid(kernel, bins, *interval)
				acc = DensityAccumulator(kernel, grid, bw if kernel in ("gaussian", "lorentzian") else 0.0, ctx=op.ctx)
			acc.update(plan)
			done += m
		if acc is None:  # (an empty shard: nothing drawn, zero statistics on the common grid)
			return np.zeros(bins), np.zeros(bins), np.zeros(2), 0, _density_grid(kernel, bins, *interval), interval, bw
		mean, m2, outside, cnt = acc.get()
	finally:
		if acc is not None:
			acc.close()
		for pl in plans.values():
			pl.close()
	return mean, m2, outside, cnt, grid, interval, bw


def _density_result(kernel, mean, m2, outside, cnt, grid, interval, bw, full: bool):
	if not full:
		return mean, grid
	stderr = np.sqrt(m2 / (cnt - 1) / cnt) if cnt > 1 else np.full_like(mean, np.inf)
	info = dict(stderr=stderr, nprobes=int(cnt), interval=tuple(interval), bw=(bw if kernel in ("gaussian", "lorentzian") else None), outside=outside, m2=m2, kernel=kernel)
	return mean, grid, info


def spectral_density(
	A, bins: int = 200, interval: Optional[tuple] = None, bw: Optional[float] = None, kernel: str = "gaussian", deg: int = 20, orth: int = 3,
	nprobes: int = 256, batch: int = 256, pdf: str = "rademacher", seed=None, full: bool = False, method: str = "lanczos",
	damping: Optional[str] = "jackson", **kwargs,
):  # fmt: skip
	"""Spectral density of A by stochastic Lanczos quadrature (Lin, Saad, Yang, SIAM Review 2016), accumulated on the GPU.

	Every probe's Gauss rule discretises psi(x; A, v) = sum_i |u_i^T v|^2 delta(x - lambda_i) (src/primate/integrate.py:30-35);
	the device smooths it with `kernel` on a fixed grid and keeps per-point (count, mean, M2) over the probes
	(engine.DensityAccumulator). `values` estimate, at the points of `grid`:
	  "gaussian" / "lorentzian": the eigenvalue count density sum_i K(x - lambda_i) (integral ~= n), bandwidth `bw`;
	  "histogram": eigenvalues per bin [e_g, e_g+1), `grid` = the bins + 1 edges;
	  "cdf": #{lambda_i < x}.
	A: anything `MatrixFunction` accepts (SciPy sparse, torch sparse CSR on the GPU, NumPy dense, a `.matvec` object,
	`TorchOperator`), or a `MatrixFunction`, whose deg / orth are then used; kwargs go to `MatrixFunction` (dtype=...).
	interval=None: the hull of the first batch's nodes, widened by INTERVAL_MARGIN of its width on each side; the grid
	is then fixed. bw=None: (b - a) / deg, the mean spacing of deg nodes over the interval.
	pdf: host draws are the columns `hutch` draws for the same seed (the `isotropic` stream); "device:<name>" draws
	Philox probe ids 0, 1, 2, ... on the GPU. full=True also returns `info`: stderr per point, nprobes, interval, bw
	and outside = the mean node mass (below, above) the grid (in eigenvalue counts).
	method="kpm": the kernel polynomial method instead (chebyshev.py) - `deg` is then the polynomial degree (deg + 1 Chebyshev
	moments from ceil(deg / 2) steps, up to 32768: no Lanczos cap, no reorthogonalisation, resolution ~ (b - a) / deg), `damping`
	("jackson": a positive kernel, "lanczos", "none") replaces kernel / bw, which must be left at their defaults, and
	interval=None means the spectral bounds (chebyshev.spectral_bounds), sampled at the midpoints of `bins` cells.
	A is then the operator itself (kwargs: dtype=...)."""
	if method not in ("lanczos", "kpm"):
		raise ValueError(f"unknown method '{method}' (one of lanczos, kpm)")
	if method == "kpm":
		if kernel != "gaussian" or bw is not None:
			raise ValueError("method='kpm' smooths by `damping`: leave kernel and bw at their defaults")
		bins, interval, _ = _density_args("gaussian", bins, interval, None, nprobes, batch, pdf)
		from .chebyshev import kpm_density

		mean, m2, outside, cnt, grid, bounds = kpm_density(A, bins, interval, deg, damping, int(nprobes), int(batch), pdf, seed, **kwargs)
		return _density_result("chebyshev", mean, m2, outside, cnt, grid, bounds, None, full)
	bins, interval, bw = _density_args(kernel, bins, interval, bw, nprobes, batch, pdf)
	from .operators import MatrixFunction

	M = A if isinstance(A, MatrixFunction) else MatrixFunction(A, deg=deg, orth=orth, **kwargs)
	res = _density_accumulate(M, kernel, bins, interval, bw, 0, int(nprobes), int(batch), pdf, seed)
	return _density_result(kernel, *res, full)
