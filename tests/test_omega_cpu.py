"""The edge recurrence of the Gram sequence on the CPU: scripts/omega_model.py runs the step as k_fin_gram
assembles it, every dot summed pairwise, with the free-running signed estimate of the distance-3 Gram entry beside the measured
one. At the committed constants the estimate stays within its radius rho, and the measured projection on the window's oldest
column stays below the certificate's bar tol / kappa - on the benchmark grids at k = 30 and on the small grids at k = 100 / 300,
where orthogonality is lost long before the run ends. Also: the C entry points exist and the model's constants are the library's."""

import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _model():
	spec = importlib.util.spec_from_file_location("omega_model", ROOT / "scripts" / "omega_model.py")
	mod = importlib.util.module_from_spec(spec)
	spec.loader.exec_module(mod)
	return mod


@pytest.mark.parametrize("kind,m,k,P", [("lap2d", 1000, 30, 6), ("lap3d", 100, 30, 4), ("lap2d", 100, 100, 6), ("lap3d", 22, 300, 4)])
def test_free_running_estimate_stays_within_its_radius(kind, m, k, P):
	om = _model()
	r = om.run_model(om.laplacian(kind, m), k, P)
	print(f"{kind}_{m} k={k}: {r}")
	assert r["steps"] == k - 3
	## the model's own figures are 0.04-0.05 for the innovation and, at c = 3.5, 0.005-0.007 for |estimate - measured| / rho: the bars
	## leave a factor of four and of fifteen, so a wrong transport coefficient or a lost term in the recurrence trips them
	assert r["est_err_over_rho"] <= 0.1, r  # |estimate - measured| well inside rho at every step, for every probe
	assert r["measured"] <= 1.0 / om.KAPPA, r  # the measured |q_{j-2} . w| never reaches the certificate's bar
	assert r["applied"] == 0, r  # ... so no projection was applied: the run IS the plain three-term recurrence
	assert r["theta_needed_c"] <= 0.2, r  # a step's innovation, in eps ||A||_inf (a step adds C = 3.5 of them to rho)


def test_constants_and_entry_points():
	om = _model()
	src = (ROOT / "primate_amd" / "csrc" / "slq.hip").read_text()
	assert float(re.search(r"constexpr double kOmegaC = ([0-9.]+);", src).group(1)) == om.C
	assert float(re.search(r"constexpr double kOmegaKappa = ([0-9.]+);", src).group(1)) == om.KAPPA
	from primate_amd import _capi

	hdr = (ROOT / "include" / "slq.h").read_text()
	for sym in ("slq_plan_window_columns", "slq_plan_window_verify", "slq_plan_window_census"):
		assert sym in _capi.EXPORTED_SYMBOLS and re.search(rf"\bint {sym}\(", hdr), sym
		assert hasattr(_capi.lib(), sym)
