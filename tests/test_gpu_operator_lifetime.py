"""An operator frees everything it owns: the bytes its device buffers hold (slq_debug_operator_device_bytes) are back where they
were once the operator is closed, for every kind of operator and every way its storage is built."""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import laplacian_2d, laplacian_3d


@pytest.fixture(scope="module")
def eng():
	from primate_amd import engine

	return engine


def _live() -> int:
	from primate_amd import _capi

	v = C.c_int64(-1)
	_capi.check(_capi.lib().slq_debug_operator_device_bytes(C.byref(v)))
	return v.value


def _weighted_nonsymmetric(A):
	rng = np.random.default_rng(11)
	c = sp.coo_matrix(A)
	W = sp.csr_matrix((rng.uniform(0.5, 1.5, c.nnz), (c.row, c.col)), shape=A.shape)
	W = (W + sp.diags(np.asarray(abs(W).sum(axis=1)).ravel() + 1.0)).tocsr()
	W.sort_indices()
	return W


def _affine():
	from primate_amd.operators import AffineOperator

	A = laplacian_2d(60)
	return AffineOperator(A, sp.diags(np.linspace(0.5, 1.5, A.shape[0])).tocsr(), t=0.25)


def _gram():
	from primate_amd.operators import GramOperator

	B = sp.random(3000, 2000, density=0.004, random_state=7, format="csr") + sp.eye(3000, 2000) * 3.0
	return GramOperator(B.tocsr())


def _dense():
	M = np.random.default_rng(3).uniform(-1.0, 1.0, (96, 96))
	return M + 96.0 * np.eye(96)  # (not symmetric: the operator keeps the transpose too)


def _kernel():
	from primate_amd.operators import KernelOperator

	return KernelOperator(np.random.default_rng(5).uniform(0.0, 1.0, (2000, 3)), "rbf", lengthscale=0.3, noise=1e-2)


class _HostDiagonal:
	"""A plugin with nothing but .matvec and .shape: the host callback operator."""

	def __init__(self, n):
		self.shape, self.dtype, self.d = (n, n), np.dtype(np.float64), np.linspace(1.0, 2.0, n)

	def matvec(self, x):
		return self.d * x


## (label, what DeviceOperator is given, the switches operator and plans are created under, probes of the plans, holds device memory,
##  then describe()["tiles"] (of every plan, or plan by plan) and ["upper_alpha"] as the commit before the owning types gave them for
##  these inputs, read off a run of that commit's library)
CASES = [
	("lap2d_150", lambda: laplacian_2d(150), {}, (130, 64, 32), True, 0, 1),
	("lap2d_150 ring tiles", lambda: laplacian_2d(150), {"SLQ_TILES": "2"}, (130, 64, 32), True, 2, 1),
	("lap2d_150 host build", lambda: laplacian_2d(150), {"SLQ_DEVICE_BUILD": "0"}, (130, 64, 32), True, 0, 1),
	("lap2d_150 ring tiles, host build", lambda: laplacian_2d(150), {"SLQ_TILES": "2", "SLQ_DEVICE_BUILD": "0"}, (130, 64, 32), True, 2, 1),
	("lap2d_150 tiles 1", lambda: laplacian_2d(150), {"SLQ_TILES": "1"}, (130, 64, 32), True, (1, 0, 0), 1),
	("lap2d_150 tiles 0", lambda: laplacian_2d(150), {"SLQ_TILES": "0"}, (130, 64, 32), True, 0, 1),
	("lap3d_24_f32", lambda: laplacian_3d(24, np.float32), {}, (130, 64), True, 0, 1),
	("lap3d_24_f32 ring tiles", lambda: laplacian_3d(24, np.float32), {"SLQ_TILES": "2"}, (130, 64), True, 2, 1),
	("lap3d_22 weighted, not symmetric", lambda: _weighted_nonsymmetric(laplacian_3d(22)), {}, (130, 64, 32), True, 0, 0),
	("lap3d_22 weighted, not symmetric, ring tiles", lambda: _weighted_nonsymmetric(laplacian_3d(22)), {"SLQ_TILES": "2"}, (130, 64, 32), True, 2, 0),
	("affine lap2d_60", _affine, {}, (32,), True, 0, 0),
	("gram 3000 x 2000", _gram, {}, (32,), True, 0, 0),
	("dense 96, not symmetric", _dense, {}, (32,), True, 0, 0),
	("kernel n=2000 d=3", _kernel, {}, (32,), True, 0, 0),
	("host callback", lambda: _HostDiagonal(500), {}, (8,), False, 0, 0),
]  # fmt: skip


def run_case(eng, make, probes, env, monkeypatch):
	"""Creates the operator and its plans (what it builds lazily is built by them), runs each plan for four steps, closes everything.
	Returns the counter after the operator, after every plan's creation, and [(tiles, upper_alpha)] of the plans."""
	for k, v in env.items():
		monkeypatch.setenv(k, v)
	op = eng.DeviceOperator(make())
	if op.kind == "affine":
		op.set_parameter(0.5)
	live, infos, plans = [_live()], [], []
	for P in probes:
		plan = eng.LanczosPlan(op, P, 4, 3)
		live.append(_live())
		info = plan.describe()
		infos.append((info["tiles"], info["upper_alpha"]))
		plan.generate_probes("rademacher", seed=3)
		plan.run()
		assert np.all(np.isfinite(plan.tridiag()[0])), P
		plans.append(plan)
	for plan in plans:
		plan.close()
	op.close()
	return live, infos


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_closing_an_operator_returns_every_byte(eng, monkeypatch, case):
	"""The issue behind this test lists lap2d_150 `under default switches, with plans at 130, 64 and 32 probes so that both merged
	streams and their upper halves exist`, and asks that the counter grow between the 64-probe plan and the 32-probe one. With
	default switches an operator below 65536 rows gets no tiles (slq_layout.hpp: layout_prefilter), so no stream exists there:
	every CSR case is therefore run as listed AND with SLQ_TILES=2 (ring-sized tiles from 4096 rows on), and the growth is asserted
	where the streams exist. (The barrier tiles of SLQ_TILES=1 serve wide panels only: the 130-probe plan reports tiles = 1, the
	narrower ones 0.)"""
	name, make, env, probes, holds, tiles, upper = case
	start = _live()
	live, infos = run_case(eng, make, probes, env, monkeypatch)
	print(name, "start", start, "live", live, "infos", infos, "end", _live())
	want = [(t, upper) for t in (tiles if isinstance(tiles, tuple) else (tiles,) * len(probes))]
	assert infos == want, (name, infos)
	assert all(v > start for v in live) if holds else all(v == start for v in live), (name, start, live)
	if tiles == 2 and len(probes) == 3:  # (the 2- and 4-merged streams were added by the plans that asked for them)
		assert live[3] > live[1], (name, live)
	assert _live() == start, (name, start, _live())
