"""NumPy restatement of the spectral density accumulator (primate_amd/csrc/slq_density.hpp), used by
tests/test_density_cpu.py and tests/test_gpu_density.py to check the device against the oracle's Gauss rules."""

import numpy as np


def density_np(kernel: str, grid: np.ndarray, bw, nodes: np.ndarray, weights: np.ndarray, vnorm2: np.ndarray) -> tuple:
	"""Per-probe values phi[p, g] = ||v_p||^2 sum_k tau_pk K(x_g, theta_pk) and the node mass outside[p] = (below, above)
	the grid, for one Gauss rule per probe (nodes, weights: P x k)."""
	th = np.asarray(nodes, dtype=np.float64)[:, None, :]
	tau = np.asarray(weights, dtype=np.float64)[:, None, :]
	vn2 = np.asarray(vnorm2, dtype=np.float64)[:, None]
	grid = np.asarray(grid, dtype=np.float64)
	if kernel == "histogram":
		lo, hi = grid[:-1][None, :, None], grid[1:][None, :, None]
		K = ((th >= lo) & (th < hi)).astype(float)
		below, above = th[:, 0, :] < grid[0], th[:, 0, :] >= grid[-1]
	else:
		x = grid[None, :, None]
		if kernel == "gaussian":
			K = np.exp(-((x - th) ** 2) / (2 * bw * bw)) / (bw * np.sqrt(2 * np.pi))
		elif kernel == "lorentzian":
			K = (bw / np.pi) / ((x - th) ** 2 + bw * bw)
		elif kernel == "cdf":
			K = (th < x).astype(float)
		else:
			raise ValueError(kernel)
		below, above = th[:, 0, :] < grid[0], th[:, 0, :] > grid[-1]
	phi = vn2 * np.sum(tau * K, axis=-1)
	w = tau[:, 0, :]
	outside = vn2 * np.stack([np.sum(w * below, axis=-1), np.sum(w * above, axis=-1)], axis=1)
	return phi, outside
