"""Randomised parity sweep on the GPU box: random SPD graphs / grids, every panel geometry, orth 0..deg,
both dtypes, against the CPU oracle on identical probes. Prints one line per failure and a summary.
usage: python scripts/fuzz_parity.py [seconds] [seed] [tiles] [omega [cases]]
`tiles`: operators big enough for workgroup tiles (n 4,100-45,000, SLQ_TILES=2 forced), panels of 16, 32 and 64 lanes per
row (17-300 probes: k_ring_pass on merged tiles and k_csr_ring_pass), orth up to k (the 8-wave form for 4..8 ring columns) -
the ring-fed tile kernels with ragged tile counts, short last (merged) tiles, empty and long rows.
`omega` (with `tiles`): the edge recurrence of the Gram sequence on the same operators at orth = 3, device only -
every case runs under SLQ_OMEGA=2 (verify: zero violations is the condition, and the results are bitwise those of SLQ_OMEGA=0) and
under the default (bitwise SLQ_OMEGA=0 where no rescue happened, else alpha / beta within 1e-10 / 3e-4 of it); stops after `cases` cases.
usage: python scripts/fuzz_parity.py [seconds] [seed] dense [cases]
`dense`: the dense operator's product kernels (tests/test_gpu_dense.py draws from the same lists): n in [1, 600], P in [1, 300], a dtype and one
variant of the SLQ_DENSE_* switches per case; the kernel the plan reports must be the expected one, the product of integer operands must equal
the exact one bit for bit (a non-symmetric A, C- or F-ordered), and a Lanczos run on B B^T / n + I (k = min(12, n), orth 0 or 3, Rademacher probes)
must give the oracle's log quadrature for every column and its alpha / beta on six columns within 1e-10 (fp64) / 3e-4 (fp32)."""
import os, sys, time
from pathlib import Path
import numpy as np, scipy.sparse as sp
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import laplacian_2d, laplacian_3d
from oracle import oracle
from primate_amd import engine as eng

oracle.build()
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
TILES = len(sys.argv) > 3 and sys.argv[3] == "tiles"
OMEGA = TILES and len(sys.argv) > 4 and sys.argv[4] == "omega"
OMEGA_CASES = int(sys.argv[5]) if len(sys.argv) > 5 else 10000
if TILES:
	os.environ["SLQ_TILES"] = "2"
tiled_cases = 0
om = {"offered": 0, "read": 0, "rescues": 0, "violations": 0, "transitions": 0, "innovation": 0.0, "margin": float("inf"), "plans_offering": 0, "plans_checked": 0, "with_rescue": 0}


def omega_case(Ad, X, deg):
	"""One operator at orth = 3 under SLQ_OMEGA = 2, 0 and the default; returns whether the case failed."""
	op = eng.DeviceOperator(Ad)
	res = {}
	for mode in ("2", "0", "1"):
		os.environ["SLQ_OMEGA"] = mode
		pl = eng.LanczosPlan(op, X.shape[1], deg, 3)
		pl.set_probes(X)
		pl.run()
		res[mode] = (*pl.tridiag(), pl.quadrature("exp", t=-0.1), pl.window_columns(), pl.window_verify(), pl.describe()["omega"])
		pl.close()
	del os.environ["SLQ_OMEGA"]
	op.close()
	same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
	v, off, on = res["2"], res["0"], res["1"]
	bad = not same(v, off) or v[4]["violations"] != 0
	if on[4]["rescues"] == 0:
		bad = bad or not same(on, off)
	else:
		tol = 1e-10 if Ad.dtype == np.float64 else 3e-4
		bad = bad or any(np.max(np.abs(x - y)) > tol * max(np.max(np.abs(y)), 1e-300) for x, y in zip(on[:2], off[:2]))
		om["with_rescue"] += 1
	for k in ("offered", "read", "rescues", "transitions"):
		om[k] += on[4][k]
	om["violations"] += v[4]["violations"]
	om["innovation"] = max(om["innovation"], v[5]["innovation"])
	om["margin"] = min(om["margin"], v[5]["margin"])
	om["plans_offering"] += on[6] == 1
	om["plans_checked"] += v[5]["innovation"] > 0.0  # (the verify run carried an estimate over a skipped step and compared it with the measurement)
	if bad:
		print(f"FAIL omega n={Ad.shape[0]} nnz={Ad.nnz} dtype={Ad.dtype} P={X.shape[1]} deg={deg}: verify {v[4]} {v[5]} default {on[4]}", flush=True)
	return bad


def dense_sweep(budget, rng, max_cases):
	"""The `dense` mode; returns the exit status."""
	from test_gpu_dense import F32, F64, SWITCHES, V32, V64, KERNEL_NAMES, expected_path

	t0 = time.time(); cases = fails = skipped = 0
	seen = {}
	worst = {"float64": 0.0, "float32": 0.0}
	while time.time() - t0 < budget and cases < max_cases:
		dtype = F64 if rng.random() < 0.7 else F32
		variant = (V64 if dtype == F64 else V32)[int(rng.integers(0, len(V64 if dtype == F64 else V32)))]
		n, P = int(rng.integers(1, 601)), int(rng.integers(1, 301))
		orth = int(rng.choice([0, 3]))
		for k in SWITCHES:
			os.environ.pop(k, None)
		os.environ.update(variant)
		what = f"n={n} P={P} dtype={np.dtype(dtype).name} variant={variant} orth={orth}"
		try:
			want_k, want_ks = expected_path(dtype, variant, n, P)
			## (a) integer operands: every partial sum is an exact float (below 2^53 / 2^24), so the BLAS product in fp64 is the exact one too
			lim = 1000 if dtype == F64 else 64
			A = rng.integers(-lim, lim + 1, (n, n)).astype(dtype)
			X = rng.integers(-lim, lim + 1, (n, P)).astype(dtype)
			op = eng.DeviceOperator(np.asfortranarray(A) if rng.random() < 0.5 else np.ascontiguousarray(A))
			pl = eng.LanczosPlan(op, P, 1, 0)
			d = pl.describe()
			pl.close()
			Y = op.matmat(X)
			op.close()
			bad = d["dense_kernel"] != want_k or (d["dense_ksplit"] != want_ks if want_ks is not None else not 1 <= d["dense_ksplit"] <= 16)
			if bad:
				print(f"FAIL dense path {what}: kernel {d['dense_kernel']} ksplit {d['dense_ksplit']}, expected {want_k} / {want_ks}", flush=True)
			exact = A.astype(np.float64) @ X.astype(np.float64)
			if not np.array_equal(Y, exact):
				w = np.argwhere(Y != exact)
				print(f"FAIL dense exact {what} kernel={want_k}: {len(w)} entries differ, rows {w[:, 0].min()}..{w[:, 0].max()}, columns {w[:, 1].min()}..{w[:, 1].max()}", flush=True)
				bad = True
			## (c) the fused epilogue and the alpha partials through Lanczos
			B = rng.standard_normal((n, n))
			S = B @ B.T / n + np.eye(n)
			S = np.asfortranarray(((S + S.T) / 2).astype(dtype))
			V = np.asfortranarray((np.floor(rng.random((n, P)) * 2) * 2 - 1).astype(dtype))
			deg = min(12, n)
			bar = 1e-10 if dtype == F64 else 3e-4
			op = eng.DeviceOperator(S)
			pl = eng.LanczosPlan(op, P, deg, orth)
			bad = bad or pl.describe()["dense_kernel"] != want_k
			pl.set_probes(V)
			pl.run()
			a, b, st = pl.tridiag()
			q = pl.quadrature("log")
			pl.close()
			op.close()
			ref = oracle.quad_batch(S, V, deg, orth, fun="log", fresh_q=True, nthreads=16)
			err = 0.0
			for c in sorted({0, P // 2, P - 1, min(P - 1, 63), min(P - 1, 64), min(P - 1, 128)}):
				al, be, Q = np.zeros(deg + 1, dtype), np.zeros(deg + 1, dtype), np.zeros((n, max(orth, 2)), dtype, order="F")
				steps = oracle.lanczos(S, V[:, c].copy(), deg, 1e-8, min(orth, deg), al, be, Q)
				if steps < deg or (deg > 1 and np.min(np.abs(be[1:deg])) < 1e-3 * np.max(np.abs(be[1:deg]))):
					skipped += 1  # (near breakdown: 1 / beta amplifies any implementation's rounding, as in the sparse sweep)
					continue
				scale = float(np.max(np.abs(al[:deg])))
				err = max(err, float(np.max(np.abs(a[c, :deg] - al[:deg])) / scale), float(np.max(np.abs(b[c, :deg] - be[:deg])) / scale), abs(float(q[c] / ref[c]) - 1.0))
				bad = bad or st[c] != steps
			if not err <= bar:
				print(f"FAIL dense lanczos {what} kernel={want_k}: error {err:.3e} above {bar:g}", flush=True)
				bad = True
			worst[np.dtype(dtype).name] = max(worst[np.dtype(dtype).name], err)
			seen[want_k] = seen.get(want_k, 0) + 1
		except Exception as e:  # noqa: BLE001
			print(f"FAIL dense {what}: {e!r}", flush=True)
			bad = True
		cases += 1
		fails += bool(bad)
		if cases % 250 == 0:
			print(f"... {cases} cases, {fails} failures, {time.time() - t0:.0f} s", flush=True)
	per = ", ".join(f"{KERNEL_NAMES[k]} {c}" for k, c in sorted(seen.items()))
	print(f"dense: {cases} cases in {time.time() - t0:.0f} s, {fails} failures ({skipped} near-breakdown columns not compared); cases per kernel: {per}; "
	      f"worst alpha / beta / log-quadrature error fp64 {worst['float64']:.2e} (bar 1e-10), fp32 {worst['float32']:.2e} (bar 3e-4)")
	return 1 if fails else 0


if len(sys.argv) > 3 and sys.argv[3] == "dense":
	sys.exit(dense_sweep(budget, rng, int(sys.argv[4]) if len(sys.argv) > 4 else 1 << 30))


def random_spd(n, deg, rng):
	m = int(n * deg / 2)
	i, j = rng.integers(0, n, m), rng.integers(0, n, m)
	W = sp.coo_matrix((rng.uniform(0.1, 1.0, m), (i, j)), shape=(n, n)).tocsr()
	W = W + W.T
	A = (sp.diags(np.asarray(abs(W).sum(axis=1)).ravel() + rng.uniform(0.05, 1.0, n)) - W).tocsr()
	A.sort_indices()
	return A

t0 = time.time(); cases = fails = 0
illposed_skipped = sensitive_skipped = lost_orth_skipped = 0
worst = 0.0
while time.time() - t0 < budget:
	kind = rng.integers(0, 4)
	if TILES:
		if kind == 0:
			A = laplacian_2d(int(rng.integers(65, 210)))
		elif kind == 1:
			A = laplacian_3d(int(rng.integers(17, 35)))
		elif kind == 2:  # banded with random gaps: rows of 1-9 nonzeros, some empty off-diagonals
			n0 = int(rng.integers(4100, 45000))
			offs = np.unique(rng.integers(1, 40, int(rng.integers(1, 5))))
			S = sp.diags([-rng.uniform(0.0, 1.0, n0 - o) * (rng.random(n0 - o) < 0.8) for o in offs], offs, shape=(n0, n0))
			S = (S + S.T).tocsr()
			A = (S + sp.diags(np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(0.05, 1.0, n0))).tocsr()
			A.eliminate_zeros()
			A.sort_indices()
		else:
			A = random_spd(int(rng.integers(4100, 20000)), float(rng.uniform(1.0, 3.0)), rng)
	elif kind == 0:
		A = laplacian_2d(int(rng.integers(6, 60)))
	elif kind == 1:
		A = laplacian_3d(int(rng.integers(4, 14)))
	else:
		A = random_spd(int(rng.integers(30, 5000)), float(rng.uniform(1.0, 12.0)), rng)
	n = A.shape[0]
	dtype = np.float64 if rng.random() < 0.7 else np.float32
	P = int(rng.choice([1, 2, 3, 7, 16, 17, 33, 64, 65, 128, 129, 200, 257]))
	if TILES:
		P = int(rng.choice([17, 20, 32, 33, 40, 64, 65, 128, 129, 200, 257])) if dtype == np.float64 else int(rng.choice([33, 40, 64, 65, 100, 128, 129, 256, 257, 300]))
	deg = int(rng.integers(1, min(n, (150 if rng.random() < 0.25 else 20) if TILES else 40) + 1))  # (tiles: a quarter of the cases run long recurrences, r04)
	orth = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, deg]))
	fun, kw = [("log", {}), ("exp", {"t": -0.1}), ("identity", {}), ("sqrt", {}), ("inv", {})][int(rng.integers(0, 5))]
	Ad = A.astype(dtype)
	X = np.asfortranarray((np.floor(rng.random((n, P)) * 2) * 2 - 1 if rng.random() < 0.5 else rng.standard_normal((n, P))).astype(dtype))
	if OMEGA:
		## (an operator's host analysis costs more than its runs: six draws of panel width, degree and probes per operator)
		for _ in range(6):
			fails += omega_case(Ad, X, deg)
			cases += 1
			if cases % 500 == 0 or cases == OMEGA_CASES:
				print(f"... {cases} cases, {fails} failures, {time.time() - t0:.0f} s: {om}", flush=True)
			if cases >= OMEGA_CASES:
				break
			P = int(rng.choice([17, 20, 32, 33, 40, 64, 65, 128, 129, 200, 257])) if dtype == np.float64 else int(rng.choice([33, 40, 64, 65, 100, 128, 129, 256, 257, 300]))
			deg = int(rng.integers(1, min(n, 150 if rng.random() < 0.25 else 20) + 1))
			X = np.asfortranarray((np.floor(rng.random((n, P)) * 2) * 2 - 1 if rng.random() < 0.5 else rng.standard_normal((n, P))).astype(dtype))
		if cases >= OMEGA_CASES:
			break
		continue
	## near-breakdown runs (beta -> 0: small grids with repeated eigenvalues) amplify rounding by 1/beta in ANY
	## implementation, and a zero Ritz value makes sqrt/log/inv a coin toss: compare only well-posed runs
	al, be, Qr = np.zeros(deg + 1, dtype), np.zeros(deg + 1, dtype), np.zeros((n, max(orth, 2)), dtype, order="F")
	steps = oracle.lanczos(Ad, X[:, 0].copy(), deg, 1e-8, min(orth, deg), al, be, Qr)
	if steps < deg or (deg > 1 and np.min(np.abs(be[1:deg])) < 1e-3 * np.max(np.abs(be[1:deg]))):
		continue
	try:
		op = eng.DeviceOperator(Ad)
		if TILES:
			pl = eng.LanczosPlan(op, P, deg, orth)
			tiled_cases += pl.describe()["tiles"] == 2
			pl.close()
		got = eng.quad_batch(op, X, deg, orth, fun=fun, **kw)
		ref = oracle.quad_batch(Ad, X, deg, orth, fun=fun, fresh_q=True, prefer="csr", **kw)
		op.close()
		err = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300))
		tol = 1e-7
		if dtype == np.float32:
			## fp32 noise is amplified by log/inv of small Ritz values: the yardstick is how far the fp32 ORACLE is
			## from the fp64 oracle on the same probes, not a fixed number
			ref64 = oracle.quad_batch(A, X.astype(np.float64), deg, orth, fun=fun, fresh_q=True, prefer="csr", **kw)
			noise = np.max(np.abs(ref - ref64) / np.maximum(np.abs(ref64), 1e-300))
			err = np.max(np.abs(got - ref64) / np.maximum(np.abs(ref64), 1e-300))
			tol = max(3e-4, 4.0 * noise)
		bad = not np.all(np.isfinite(got) == np.isfinite(ref)) or not (err <= tol or not np.isfinite(err))
		if np.isfinite(err):
			worst = max(worst, err if dtype == np.float64 else 0.0)
	except Exception as e:  # noqa: BLE001
		bad, err = True, repr(e)
	cases += 1
	if bad and not isinstance(err, str):
		## the pre-filter looked at probe 0 only: a mismatch confined to probes whose own run is near breakdown
		## (beta collapsing to the stop tolerance) is the ill-posed case again, not a failure
		rel = np.abs(got - (ref64 if dtype == np.float32 else ref)) / np.maximum(np.abs(ref), 1e-300)
		offenders = np.flatnonzero(~np.isfinite(got) | ~np.isfinite(ref) | ~(rel <= tol))
		def ill_posed(c):
			a1, b1, Q1 = np.zeros(deg + 1, dtype), np.zeros(deg + 1, dtype), np.zeros((n, max(orth, 2)), dtype, order="F")
			st = oracle.lanczos(Ad, X[:, c].copy(), deg, 1e-8, min(orth, deg), a1, b1, Q1)
			return st < deg or (deg > 1 and np.min(np.abs(b1[1:deg])) < 1e-3 * np.max(np.abs(b1[1:deg])))
		if len(offenders) and all(ill_posed(int(c)) for c in offenders[:20]):
			bad = False
			illposed_skipped += 1
		elif np.all(np.isfinite(got)) and np.all(np.isfinite(ref)):
			## conditioning: how far does the ORACLE move when the probes change in their last bit? (partial
			## reorthogonalisation with many steps + inv/log of small Ritz values amplifies rounding by 1e8 and more)
			Xp = np.asfortranarray((X * (1 + np.finfo(dtype).eps * np.sign(rng.standard_normal(X.shape)))).astype(dtype))
			refp = oracle.quad_batch(Ad, Xp, deg, orth, fun=fun, fresh_q=True, prefer="csr", **kw)
			sens = np.max(np.abs(refp - ref) / np.maximum(np.abs(ref), 1e-300))
			if np.nanmax(rel) <= 10.0 * sens:
				bad = False
				sensitive_skipped += 1
				print(f"note: kind={kind} n={n} P={P} deg={deg} orth={orth} fun={fun}: err {np.nanmax(rel):.2e} within 10x the oracle's own 1-ulp sensitivity {sens:.2e}", flush=True)
			elif orth < deg:
				## a partial window that has LOST orthogonality (r04, seed 22 case 4705: n = 1488, k = 37, orth = 1 - alpha of any two implementations parts ways at
				## step 25 by O(1), the quadrature moves by 1e-7): the value is determined no better than the distance between the oracle's own partial-
				## and full-reorthogonalisation runs on the same probes, per probe - but never above north_star's 1e-6: a miss
				## beyond that counts as a failure whatever the spread (tests/test_gpu_parity.py pins this class of case)
				ref_full = oracle.quad_batch(Ad, X, deg, deg, fun=fun, fresh_q=True, prefer="csr", **kw)
				spread = np.abs(ref_full - ref) / np.maximum(np.abs(ref), 1e-300)
				if np.all(rel <= np.maximum(3.0 * spread, tol)) and np.all(rel <= 1e-6):
					bad = False
					lost_orth_skipped += 1
					print(f"note: kind={kind} n={n} P={P} deg={deg} orth={orth} fun={fun}: err {np.nanmax(rel):.2e} within 3x the oracle's partial-vs-full reorthogonalisation spread {np.max(spread):.2e}", flush=True)
	if bad:
		fails += 1
		try:  # keep the inputs of a failing case for a post-mortem
			out = ROOT / "gpurun_out"
			out.mkdir(exist_ok=True)
			Ac = A.tocsr()
			np.savez(out / f"fuzz_fail_{cases}.npz", indptr=Ac.indptr, indices=Ac.indices, data=Ac.data, n=n, X=X, deg=deg, orth=orth, fun=fun,
			         dtype=str(np.dtype(dtype)), got=got, ref=ref)
		except Exception:  # noqa: BLE001
			pass
		print(f"FAIL kind={kind} n={n} nnz={A.nnz} dtype={dtype.__name__} P={P} deg={deg} orth={orth} fun={fun} err={err}", flush=True)
	if cases % 50 == 0:
		print(f"... {cases} cases, {fails} failures, worst fp64 rel err {worst:.2e}, {time.time() - t0:.0f} s", flush=True)
if OMEGA:
	print(f"omega: {cases} cases (deg <= 150, orth = 3), {fails} failures, {om['violations']} violations; {om['plans_offering']} plans offered their windows, {om['plans_checked']} compared an estimate with a measurement in verify mode (the others are too small to skip: tol / kappa below three theta): "
	      f"{om['read']} of {om['offered']} columns read, {om['rescues']} rescues in {om['with_rescue']} cases, {om['transitions']} read -> skip transitions; "
	      f"largest innovation {om['innovation']:.4f} eps ||A||_inf, smallest margin {om['margin']:.3f}")
	sys.exit(1 if fails or om["violations"] else 0)
if TILES:
	print(f"{tiled_cases} of the {cases} cases ran on ring-fed tiles")
print(f"done: {cases} cases, {fails} failures ({illposed_skipped} mismatches confined to near-breakdown probes, {sensitive_skipped} within 10x the oracle's own 1-ulp sensitivity and "
      f"{lost_orth_skipped} within 3x its partial-vs-full reorthogonalisation spread not counted), worst fp64 rel err {worst:.2e}")
sys.exit(1 if fails else 0)
