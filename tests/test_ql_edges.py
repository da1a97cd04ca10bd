"""The hand-written tridiagonal QL at its edges, against a 50-digit reference.

Two copies of the implicit-shift QL serve every rule the engine returns: k_quadrature carries only the first
row of the eigenvector matrix, ql_implicit_full (k_eigh_tridiag, k_fun_coeffs) the whole matrix, in LDS up to
k = 141 and in a global scratch above. `edge_cases()` is the input set and `reference()` a plain function from
(d, e) to its mpmath reference, so the same set runs twice: against the oracle's C QL (oracle.tridiag_ql, the
same textbook algorithm) on every CPU run, which checks the set and its tolerances, and against the device
(`-m gpu`), all cases of one size in one batch so that lanes need very different iteration counts.

Bars (C_NODE = 4): nodes within C_NODE k eps ||T||; weights summed over clusters of nodes closer than
1e3 eps ||T|| to 1e-13; sum f(theta) tau equal to e1^T f(T) e1 to 1e-12 of sum |f(theta)| tau; f(T) e1 of the
action path to 1e-12 of its largest absolute sum, max_i sum_j |v_ij f(lambda_j) v_0j|; eigenvectors orthonormal
to 1e-13 with ||T Z - Z Lambda|| <= C_NODE k eps ||T||; no convergence failure. A subnormal T has fewer digits:
its bars grow by 5e-324 / (eps ||T||).
"""

import functools

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
C_NODE = 4  # nodes, residuals: within C_NODE * k * eps * ||T||
W_TOL, F_TOL, ORTH_TOL = 1e-13, 1e-12, 1e-13
MP_DIGITS = 50


def _toeplitz(k, c, b):
	d, e = np.full(k, float(c)), np.full(k, float(b))
	e[0] = 0.0
	return d, e


def _random(rng, k):
	d, e = rng.uniform(-1.0, 1.0, k), rng.uniform(0.1, 1.0, k)
	e[0] = 0.0
	return d, e


def _split_toeplitz(rng, k, nsplit):
	"""Constant blocks of random sizes (each block its own diagonal and coupling), cut by exact zero couplings."""
	cuts = np.sort(rng.choice(np.arange(1, k), size=min(nsplit, k - 1), replace=False)) if k > 1 else np.zeros(0, dtype=int)
	d, e = np.zeros(k), np.zeros(k)
	for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, k]):
		d[lo:hi] = rng.uniform(-3.0, 3.0)
		e[lo + 1 : hi] = rng.uniform(0.2, 2.0) * rng.choice([-1.0, 1.0])
	return d, e


def _pad(d, e, k):
	return np.r_[d, np.zeros(k - len(d))], np.r_[e, np.zeros(k - len(e))]


def edge_cases():
	"""{k: [(name, d, e), ...]}: e[i] couples i-1 and i, e[0] = 0 (the engine's layout). Every size is one device batch,
	padded with split Toeplitz matrices (closed-form references) to nb in {63, 65, 129} where it holds several cases."""
	rng = np.random.default_rng(20261016)
	C = {k: [] for k in (1, 2, 3, 32, 64, 141, 142, 300)}
	## k = 1 and 2: scalars and 2 x 2 blocks, signs, zeros and extreme scales
	for v in (0.0, 1.0, -2.5, 1e150, -1e-150, 5e-324):
		C[1].append((f"scalar {v:g}", np.array([v]), np.zeros(1)))
	for name, d, b in [("2x2 equal diagonal", (1.0, 1.0), 1e-8), ("2x2 zero diagonal", (0.0, 0.0), 3.0), ("2x2 decoupled", (2.0, -1.0), 0.0),
	                   ("2x2 tiny coupling", (1.0, 1.0 + 4 * EPS), 1e-300), ("2x2 huge", (1e150, -1e150), 1e150), ("2x2 graded", (1e-8, 1e8), 1.0)]:  # fmt: skip
		C[2].append((name, np.array(d, dtype=np.float64), np.array([0.0, b])))
	## 1-D Laplacians: nodes 2 - 2cos(j pi/(k+1)), weights 2/(k+1) sin^2(j pi/(k+1))
	for k in C:
		if k > 1:
			C[k].append((f"1-D Laplacian {k}", *_toeplitz(k, 2.0, -1.0)))
	C[3].append(("3x3 zero diagonal", np.zeros(3), np.array([0.0, 1.0, 1.0])))
	C[3].append(("3x3 negative definite", *_toeplitz(3, -4.0, 1.0)))
	## irregular cases (mpmath's eigensolver)
	for k in (32, 64):
		C[k].append((f"random indefinite {k}", *_random(rng, k)))
		d, e = _random(rng, k)
		C[k].append((f"zero diagonal {k}", np.zeros(k), e))
		d, e = _random(rng, k)
		e[rng.choice(np.arange(2, k - 1), 3, replace=False)] = 0.0  # exact zero couplings: block splits
		C[k].append((f"interior zero couplings {k}", d, e))
		d, e = _random(rng, k)
		d[k // 2 :], e[k // 2 :] = 0.0, 0.0  # the zero tail after an early stop
		C[k].append((f"zero tail {k}", d, e))
		d, e = _random(rng, k)
		e[[3, k // 3, k - 2]] = 1e-300
		C[k].append((f"couplings 1e-300 {k}", d, e))
		d, e = _random(rng, k)
		for j, fac in ((5, 1.0), (k // 2, 0.5), (k - 3, 2.0)):  # at, below and above the deflation test |e_m| <= eps (|d_m| + |d_m+1|)
			e[j] = fac * EPS * (abs(d[j - 1]) + abs(d[j]))
		C[k].append((f"couplings at the deflation threshold {k}", d, e))
		d = 10.0 ** np.linspace(-8.0, 8.0, k)
		e = np.r_[0.0, 0.5 * np.sqrt(d[1:] * d[:-1])]
		C[k].append((f"graded 1e-8..1e8 {k}", d, e))
		C[k].append((f"graded 1e8..1e-8 {k}", d[::-1].copy(), np.r_[0.0, e[1:][::-1]]))
		d, e = _random(rng, k)
		C[k].append((f"scale 1e150 {k}", d * 1e150, e * 1e150))
		C[k].append((f"scale 1e-150 {k}", d * 1e-150, e * 1e-150))
		L = _toeplitz(k, 2.0, -1.0)
		C[k].append((f"negative definite {k}", -L[0] - 0.1, -L[1]))
	for m, k in ((10, 32), (20, 64)):  # Wilkinson W+_{2m+1}: pairs of eigenvalues that agree to many digits (zero-padded)
		d, e = np.abs(np.arange(2 * m + 1) - m).astype(np.float64), np.ones(2 * m + 1)
		e[0] = 0.0
		C[k].append((f"Wilkinson W+ {2 * m + 1} in {k}", *_pad(d, e, k)))
	## subnormal entries: a rotation whose f and g both underflow to zero (the QL's r == 0 branch)
	d, e = np.array([2.17e-322, 0.0, 1.09e-322, 4.35e-322, 0.0]), np.array([0.0, 2.17e-322, 1.09e-322, 2.17e-322, 1.09e-322])
	C[32].append(("subnormal 5 in 32", *_pad(d, e, 32)))
	## large k: split Laplacians and zero tails (closed forms), the LDS / global boundary of the eigenvector kernels
	for k in (141, 142, 300):
		d, e = _toeplitz(k, 2.0, -1.0)
		e[[k // 5, k // 2, k // 2 + 1, k - 10]] = 0.0
		C[k].append((f"split Laplacian {k}", d, e))
		d, e = _toeplitz(k, 2.0, -1.0)
		d[k - 37 :], e[k - 37 :] = 0.0, 0.0
		C[k].append((f"Laplacian with zero tail {k}", d, e))
		C[k].append((f"Toeplitz 1e-150 {k}", *_toeplitz(k, 1e-150, 2e-150)))
	## pad to batch sizes that straddle wavefronts and workgroups
	for k, nb in ((1, 65), (2, 63), (3, 129), (32, 63), (64, 65)):
		while len(C[k]) < nb:
			C[k].append((f"split Toeplitz {k} #{len(C[k])}", *_split_toeplitz(rng, k, int(rng.integers(0, min(k, 6))))))
	C[141] = C[141][:1]  # nb = 1 at the last on-chip size
	return C


def _blocks(d, e):
	"""Index ranges of the blocks that exact zero couplings cut T into."""
	cuts = [i for i in range(1, len(d)) if e[i] == 0.0]
	return list(zip([0] + cuts, cuts + [len(d)]))


@functools.lru_cache(maxsize=None)
def _reference_cached(key):
	import mpmath as mp

	d, e = (np.frombuffer(b) for b in key)
	k = len(d)
	mp.mp.dps = MP_DIGITS
	lam, cols = [], []  # eigenvalues and their eigenvectors (lists of k mpf)
	for lo, hi in _blocks(d, e):
		m = hi - lo
		db, eb = d[lo:hi], e[lo + 1 : hi]
		if np.all(db == db[0]) and (m == 1 or np.all(eb == eb[0])):
			## constant diagonal c and coupling b: c + 2b cos(j pi/(m+1)), sqrt(2/(m+1)) sin(i j pi/(m+1))
			c, b = mp.mpf(float(db[0])), (mp.mpf(float(eb[0])) if m > 1 else mp.mpf(0))
			for j in range(1, m + 1):
				lam.append(c + 2 * b * mp.cos(j * mp.pi / (m + 1)))
				v = [mp.mpf(0)] * k
				for i in range(m):
					v[lo + i] = mp.sqrt(mp.mpf(2) / (m + 1)) * mp.sin((i + 1) * j * mp.pi / (m + 1))
				cols.append(v)
		else:
			assert m <= 64, "the mpmath eigensolver is for the small irregular blocks"
			M = mp.zeros(m, m)
			for i in range(m):
				M[i, i] = mp.mpf(float(db[i]))
				if i + 1 < m:
					M[i, i + 1] = M[i + 1, i] = mp.mpf(float(eb[i]))
			E, Q = mp.eigsy(M)
			for j in range(m):
				lam.append(E[j])
				v = [mp.mpf(0)] * k
				for i in range(m):
					v[lo + i] = Q[i, j]
				cols.append(v)
	order = sorted(range(k), key=lambda j: lam[j])
	lam, cols = [lam[j] for j in order], [cols[j] for j in order]
	w = [v[0] ** 2 for v in cols]
	norm = max(abs(x) for x in lam)
	out = {"nodes": np.array([float(x) for x in lam]), "weights": np.array([float(x) for x in w]), "norm": float(norm), "fun": {}, "action": {}}
	## e1^T f(T) e1 (with sum |f(lambda)| w, the scale it is held to) and f(T) e1, where they are finite in fp64
	fs = {"identity": lambda x: x}
	if mp.mpf("1e-100") < norm < mp.mpf("1e100"):
		fs["exp"] = mp.exp
		if (min(lam) > 0 or max(lam) < 0) and norm / min(abs(x) for x in lam) <= 1e4:  # (1/theta of an ill-conditioned T tests the conditioning, not the QL)
			fs["inv"] = lambda x: 1 / x
	for f, fn in fs.items():
		vals = [fn(x) for x in lam]
		s, sa = mp.fsum(v * t for v, t in zip(vals, w)), mp.fsum(abs(v) * t for v, t in zip(vals, w))
		if sa < mp.mpf("1e300"):
			out["fun"][f] = (float(s), float(sa))
			y = [mp.fsum(cols[j][i] * vals[j] * cols[j][0] for j in range(k)) for i in range(k)]
			ya = max(mp.fsum(abs(cols[j][i] * vals[j] * cols[j][0]) for j in range(k)) for i in range(k))
			out["action"][f] = (np.array([float(v) for v in y]), float(ya))
	return out


def reference(d, e):
	"""The 50-digit reference of T(d, e): ascending nodes, first-row weights, ||T||, e1^T f(T) e1 with the absolute sum
	sum |f(lambda)| w it is measured against, and f(T) e1 with the largest absolute sum max_i sum_j |v_ij f(lambda_j) v_0j|. Exact zero couplings cut T into blocks; a block with constant
	diagonal and coupling takes the closed form, any other block mpmath's symmetric eigensolver."""
	return _reference_cached((np.ascontiguousarray(d, dtype=np.float64).tobytes(), np.ascontiguousarray(e, dtype=np.float64).tobytes()))


def _clusters(nodes, tol):
	"""Index groups of ascending nodes closer than tol to their neighbour."""
	groups, cur = [], [0]
	for i in range(1, len(nodes)):
		if nodes[i] - nodes[i - 1] < tol:
			cur.append(i)
		else:
			groups.append(cur)
			cur = [i]
	groups.append(cur)
	return groups


def _norm(R):
	return max(R["norm"], np.finfo(np.float64).tiny)


def _grow(R):
	"""1, or how much coarser than eps numbers of the size of ||T|| are when they are subnormal (5e-324 / ||T||)."""
	return max(1.0, 5e-324 / max(R["norm"], 5e-324) / EPS)


def check_rule(name, d, e, nodes, weights, quad, worst):
	"""Ascending nodes and weights of T(d, e), and quad = {f: sum f(theta) tau}, against reference()."""
	R = reference(d, e)
	k = len(d)
	ratio = np.max(np.abs(nodes - R["nodes"])) / (k * EPS * _grow(R) * max(R["norm"], 5e-324))
	worst["node"] = max(worst["node"], ratio)
	assert ratio <= C_NODE, f"{name}: node error {ratio:.2f} k eps ||T|| (bar {C_NODE})"
	groups = _clusters(R["nodes"], 1e3 * EPS * _norm(R))
	for c, g in enumerate(groups):
		ws, wr = np.sum(weights[g]), np.sum(R["weights"][g])
		## a cluster whose neighbour is near (Wilkinson pairs) has ill-conditioned weights: Davis-Kahan, sin(angle) <= ||E|| / gap
		## with a backward error ||E|| of C_NODE eps ||T||, moves them by 2 |z| sin + sin^2; elsewhere the bar is W_TOL
		gap = np.inf
		if c > 0:
			gap = R["nodes"][g[0]] - R["nodes"][groups[c - 1][-1]]
		if c + 1 < len(groups):
			gap = min(gap, R["nodes"][groups[c + 1][0]] - R["nodes"][g[-1]])
		s =C_NODE * EPS * _norm(R) / gap
		tol = max(W_TOL * _grow(R), 2.0 * np.sqrt(wr) * s + s * s)
		assert abs(ws - wr) <= tol, f"{name}: weight of the cluster at {R['nodes'][g[0]]:.6g} ({len(g)} nodes, gap {gap:.2e}) {ws!r} vs {wr!r}"
	for f, (ref, scale) in R["fun"].items():
		got = quad[f]
		scale = max(scale, np.finfo(np.float64).tiny)
		worst["fun"] = max(worst["fun"], abs(got - ref) / scale)
		assert abs(got - ref) <= F_TOL * _grow(R) * scale, f"{name}: sum {f}(theta) tau = {got!r}, e1^T {f}(T) e1 = {ref!r}"
	return R


def check_vectors(name, d, e, w, Z, worst):
	"""Eigenvectors (columns of Z) and eigenvalues w of T(d, e): orthonormal, small residual."""
	k = len(d)
	R = reference(d, e)
	T = np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1)
	orth = np.max(np.abs(Z.T @ Z - np.eye(k)))
	res = np.max(np.abs(T @ Z - Z * w[None, :])) / (k * EPS * _norm(R))
	worst["orth"], worst["resid"] = max(worst["orth"], orth / _grow(R)), max(worst["resid"], res / _grow(R))  # (in units of the bars)
	assert orth <= ORTH_TOL * _grow(R), f"{name}: |Z^T Z - I| = {orth:.2e}"
	assert res <= C_NODE * _grow(R), f"{name}: |T Z - Z Lambda| = {res:.2f} k eps ||T||"


def _sums(nodes, weights):
	with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
		return {"identity": np.sum(nodes * weights), "exp": np.sum(np.exp(nodes) * weights), "inv": np.sum(weights / nodes)}


def _report(who, worst):
	print(f"{who} QL, worst over the edge set: node {worst['node']:.3f} k eps ||T|| (bar {C_NODE}), sum f tau {worst['fun']:.2e} (bar {F_TOL}), "
	      f"|Z^T Z - I| {worst['orth']:.2e} (bar {ORTH_TOL}), residual {worst['resid']:.3f} k eps ||T|| (bar {C_NODE})")  # fmt: skip


def test_edge_set_on_the_oracle_ql(oracle):
	"""The set and its bars on the oracle's C QL (the same algorithm as both device copies), first-row and full forms."""
	worst = {"node": 0.0, "fun": 0.0, "orth": 0.0, "resid": 0.0}
	for k, cases in edge_cases().items():
		for name, d, e in cases:
			w1, z1, rc = oracle.tridiag_ql(d, e, first_row_only=True)
			assert rc == 0, f"{name}: QL did not converge"
			o = np.argsort(w1, kind="stable")
			check_rule(name, d, e, w1[o], z1[0, o] ** 2, _sums(w1[o], z1[0, o] ** 2), worst)
			wf, Z, rc = oracle.tridiag_ql(d, e, want_vectors=True)
			assert rc == 0, f"{name}: QL did not converge"
			o = np.argsort(wf, kind="stable")
			check_vectors(name, d, e, wf[o], Z[:, o], worst)
	_report("oracle", worst)


@pytest.mark.gpu
def test_edge_set_on_the_device():
	"""k_quadrature (nodes, weights, sum f tau for identity / exp / inv), k_eigh_tridiag (LDS for k <= 141, global scratch
	above) and k_fun_coeffs (fun_action_batch on the matrix T itself from e1, whose Lanczos run reproduces T up to its
	first coupling below the stop rule) on the whole set; both QL copies must give the same nodes, and neither may report a failure
	(the entries raise if one does)."""
	try:
		import mpmath  # noqa: F401
	except ImportError:  # the reference is required, not optional
		pytest.fail("mpmath is needed for the 50-digit reference of the QL edge cases")
	import scipy.sparse as sp

	from primate_amd import engine as eng

	worst = {"node": 0.0, "fun": 0.0, "orth": 0.0, "resid": 0.0}
	for k, cases in edge_cases().items():
		D = np.array([d for _, d, _ in cases])
		E = np.array([e for _, _, e in cases])
		nodes, weights = eng.quadrature_batch(D, E)
		quad = {f: eng.quadrature_batch(D, E, fun=f)[0] for f in ("identity", "exp", "inv")}
		w, Z = eng.eigh_tridiag_batch(D, E)
		for i, (name, d, e) in enumerate(cases):
			R = check_rule(name, d, e, nodes[i], weights[i], {f: quad[f][i] for f in quad}, worst)
			check_vectors(name, d, e, w[i], Z[i], worst)
			assert np.max(np.abs(w[i] - nodes[i])) <= C_NODE * k * EPS * _norm(R), f"{name}: k_eigh_tridiag and k_quadrature nodes differ"
		## the action path (k_fun_coeffs: Z in LDS up to k = 141, in a global scratch above). Lanczos on T from e1 reproduces T
		## exactly and stops after the first step m whose coupling is below sqrt(k) rtol (lanczos.h:139-142, rtol = 1e-8): the
		## result is then f(T_m) e1 of the leading m x m block, zero below it
		stop = np.sqrt(k) * 1e-8
		for name, d, e in cases[:12]:
			a = np.abs(e[1:])
			small = np.flatnonzero(a < stop)
			m = int(small[0]) + 1 if len(small) else k
			if k < 2 or not (1e-100 < reference(d, e)["norm"] < 1e100) or np.any((a[:m] > 0.5 * stop) & (a[:m] < 2.0 * stop)):
				continue  # (a coupling this close to the stop rule leaves open where the run ends)
			R = reference(d[:m], e[:m])
			T = sp.csr_matrix(np.diag(d) + np.diag(e[1:], 1) + np.diag(e[1:], -1))
			x = np.zeros(k)
			x[0] = 1.0
			op = eng.DeviceOperator(T)
			for f, (ym, scale) in R["action"].items():
				y = np.r_[ym, np.zeros(k - m)]
				got = eng.fun_action_batch(op, x, m, m, fun=f)[:, 0]
				err = np.max(np.abs(got - y)) / scale  # (held like the sums above: to F_TOL of the absolute sum, not of |f(T) e1|)
				worst["fun"] = max(worst["fun"], err)
				assert err <= F_TOL, f"{name}: f(T) e1 for f = {f}: {err:.2e}"
			op.close()
	_report("device", worst)


@pytest.mark.gpu
def test_early_stop_rule_pinned_to_the_oracle(golden, oracle):
	"""The zero-tailed T of an early stop (golden stop_A: 5 of 20 steps) through log and inv, whose f is not finite at the
	tail's zero nodes: the device's per-probe sums equal the oracle's, NaN exactly where the oracle's is NaN."""
	from primate_amd import engine as eng

	A, v = golden["stop_A"], golden["stop_v"]
	op = eng.DeviceOperator(A)
	for f in ("log", "inv", "identity"):
		got = eng.quad_batch(op, v, 20, 20, fun=f)
		ref = oracle.quad_batch(A, v, 20, 20, fun=f, fresh_q=True)
		assert np.array_equal(np.isnan(got), np.isnan(ref)), (f, got, ref)
		np.testing.assert_allclose(got, ref, rtol=1e-10, equal_nan=True, err_msg=f)
	op.close()
