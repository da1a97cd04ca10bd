"""The generators and exact models of tests/_csr_cases.py, checked on the CPU: what tests/test_gpu_csr_edges.py relies on.

 * the families have the row lengths, symmetry and row sums they are described with, and every spelling is the same matrix;
 * exact_product and exact_chebyshev agree with independent statements (a dense int64 product, a recurrence in Fractions);
 * the exactness bound of the Chebyshev model holds for every family, spelling and dtype check (b) uses, at its step count;
 * the Lanczos inputs of check (c) are insensitive: the oracle against oracle.np_lanczos over a randomly ordered scatter product of
   the same matrix stays within 1 / 100 of check (c)'s bars."""

from fractions import Fraction

import numpy as np
import pytest

import _csr_cases as cc

F64, F32 = np.float64, np.float32


def test_families_are_what_they_are_described_as():
	for name in cc.ALL_NAMES:
		for values in ("integer", "spd"):
			if values == "spd" and (name.startswith("nonsym") or name.startswith("zero")):
				continue
			M = cc.family(name, values)
			n = M.n
			D = {(int(i), int(j)): int(v) for i, j, v in zip(M.rows, M.cols, M.num)}
			assert 0 not in D.values(), name  # the canonical spelling stores no zero
			if M.symmetric:
				assert all(D.get((j, i)) == v for (i, j), v in D.items()), name
			lens = np.bincount(M.rows, minlength=n)
			sums = M.abs_row_sums()
			if values == "integer":
				assert sums.max(initial=0) <= 16, name
				if M.shift == 0:
					assert all(abs(v) == (2 if name.startswith("nonsym") else 1) for (i, j), v in D.items() if i != j) and all(1 <= abs(v) <= 2 for (i, j), v in D.items() if i == j)
			elif M.nnz:
				d = np.array([D.get((i, i), 0) for i in range(n)]) / 2.0**M.shift
				off = sums - np.abs(d)
				assert np.all((d == 0) == (lens == 0)) or name.startswith("longrow"), name
				assert np.all(d[lens > 1] >= off[lens > 1] + 1.0) and np.all(d[lens > 1] < off[lens > 1] + 1.0 + 1.0 / 64), name  # rounded up to 1 / 64, plus 1
				assert np.all((M.num / 2.0**M.shift * 1024) % 1 == 0)
			if name.startswith("band") and n >= 257:
				## (0 to 11 entries; both sides of the chunk-of-four boundaries 3/4/5 and 8/9 occur)
				assert lens.min() == 0 and 9 <= lens.max() <= 11 and set(range(3, 10)) <= set(lens.tolist()), (name, sorted(set(lens.tolist())))
			if name.startswith("band") and n >= 63:
				assert lens.min() == 0  # an emptied index
			if name.startswith("longrow"):
				_, r, L = (int(x) for x in name[7:].split("_"))
				assert lens[r] == L + 1 and np.count_nonzero(M.cols == r) == L + 1
				k = (M.rows == r) & (M.cols != r)
				assert np.all(np.abs(M.num[k]) == 1) and M.shift == 10  # +-2**-10
			if name.startswith("grid"):
				assert lens.min() >= 1 and lens.max() == 5 and 0.7 < (M.nnz - n) / (4.0 * n) < 0.8
			if name.startswith("far"):
				far = np.count_nonzero(np.abs(M.rows - M.cols) > 4096) / n
				assert (far > 4.2) if name == "far7" else (0.5 < far < 0.8), (name, far)
	assert cc.family("grid64").n == 4096 and cc.family("grid70").n == 4900 and cc.family("far").n == 8200 and cc.family("zero65").nnz == 0


def test_every_spelling_is_the_same_matrix_and_is_spelled_as_named():
	for name in cc.ALL_NAMES:
		M = cc.family(name)
		X = cc.int_panel(M.n, 5, 3)
		ref = None
		for sp in cc.SPELLINGS:
			R = cc.raw(name, sp)
			assert R.rowptr[0] == 0 and R.rowptr[-1] == R.nnz and np.all(np.diff(R.rowptr) >= 0) and R.colind.dtype == np.int32
			assert R.nnz == 0 or (R.colind.min() >= 0 and R.colind.max() < M.n)
			for dt in (F64, F32):
				R.vals(dt)  # representable (asserted inside)
			Y, _ = cc.exact_product(R, X)
			ref = Y if ref is None else ref
			assert np.array_equal(Y, ref), (name, sp)
			if M.n <= 257:
				assert np.array_equal(R.dense_num(), cc.raw(name, "canonical").dense_num()), (name, sp)
			rows, ci = R.rows, R.colind.astype(np.int64)
			same_row = rows[1:] == rows[:-1]
			step = np.diff(ci)
			if sp == "canonical":
				assert np.all(step[same_row] > 0)
			if M.nnz < 20:
				continue
			if sp == "shuffled":
				assert np.any(step[same_row] < 0) and not np.any(step[same_row] == 0)
			if sp == "reversed":
				assert np.all(step[same_row] < 0)
			if sp == "dups":
				adjacent = same_row & (step == 0)
				assert np.any(adjacent & (rows[1:] % 2 == 0)), name  # behind one another in even rows
				key = rows * M.n + ci
				order = np.argsort(key, kind="stable")
				twice = key[order][1:] == key[order][:-1]
				apart = twice & (np.diff(order) > 1)
				assert np.any(apart), name  # ... and apart in odd rows
				assert R.nnz > M.nnz * 1.3
			if sp == "zeros":
				assert np.count_nonzero(R.num == 0) >= 1
				lens0, lens1 = np.bincount(M.rows, minlength=M.n), np.bincount(rows, minlength=M.n)
				if np.any(lens0 == 0):
					i = int(np.flatnonzero(lens0 == 0)[0])
					assert lens1[i] >= 1 and np.all(R.num[rows == i] == 0 if lens1[i] == 1 else True)
				pair = same_row & (step == 0)
				assert np.any(pair) and np.all(R.num[1:][pair] == -R.num[:-1][pair])  # +v, -v at one position outside the pattern
	Z = cc.raw("zero65", "zeros")
	assert Z.nnz > 0 and not np.any(Z.dense_num())
	## the rule of the upper-triangle copy, as check (b) and (c) expect it of the library
	for name in ("band1", "band65", "grid64"):
		got = {sp: (cc.stored_exactly_symmetric(cc.raw(name, sp)), cc.stored_exactly_symmetric(cc.raw(name, sp), True)) for sp in cc.SPELLINGS}
		assert got["canonical"] == (True, True) and got["dups"] == (False, False), (name, got)
		if name != "band1":
			assert got["shuffled"] == got["reversed"] == (False, True) and got["zeros"] == (False, False), (name, got)
	assert not cc.stored_exactly_symmetric(cc.raw("nonsym65", "canonical"))


def test_exact_product_against_a_dense_int64_product():
	for name in ("band5", "band65", "nonsym65", "longrow1000_999_65", "band257"):
		M = cc.family(name)
		X = cc.int_panel(M.n, 17, 1)
		D = np.zeros(M.shape, dtype=np.int64)
		D[M.rows, M.cols] = M.num
		for sp in cc.SPELLINGS:
			Y, bits = cc.exact_product(cc.raw(name, sp), X)
			assert np.array_equal(Y * 2.0**M.shift, D @ X) and bits < 24
			if name.startswith("nonsym"):
				assert not np.array_equal(Y, D.T @ X)
	R = cc.spell(cc.rect(350, 200), "dups")
	X = cc.int_panel(200, 9, 2)
	T, b1 = cc.exact_product(R, X)
	D = np.zeros((350, 200), dtype=np.int64)
	D[R.M.rows, R.M.cols] = R.M.num
	assert np.array_equal(T, D @ X) and b1 < 24


def test_exact_chebyshev_against_a_recurrence_in_fractions():
	for name, nsteps in (("band65", 6), ("longrow1000_999_65", 3)):
		R = cc.raw(name, "dups")
		M = R.M
		n, P = M.n, 3
		V = cc.rademacher(n, P, 5)
		A = {}
		for i, j, v in zip(R.rows, R.colind, R.num):
			A.setdefault(int(i), []).append((int(j), Fraction(int(v), 2**M.shift)))
		h = Fraction(16)
		m = cc.exact_chebyshev(R, V, nsteps)
		assert m["K"] == nsteps
		for p in range(P):
			w = [[Fraction(int(x)) for x in V[:, p]]]
			for j in range(nsteps):
				Aw = [sum((a * w[j][k] for k, a in A.get(i, [])), Fraction(0)) for i in range(n)]
				w.append([x / h for x in Aw] if j == 0 else [2 * x / h - y for x, y in zip(Aw, w[j - 1])])
			for k in range(nsteps + 1):
				assert all(Fraction(float(m["w"][k][i, p])) == w[k][i] for i in range(n)), (name, k)
			mu = [sum(x * x for x in w[0]), sum(x * y for x, y in zip(w[1], w[0]))]
			for k in range(2, 2 * nsteps + 1):
				a, b = (k + 1) // 2, k // 2
				mu.append(2 * sum(x * y for x, y in zip(w[a], w[b])) - mu[k % 2])
			for k in range(2 * nsteps + 1):
				if np.isfinite(m["mu"][p, k]):
					assert Fraction(float(m["mu"][p, k])) == mu[k], (name, k)
			assert np.all(np.isfinite(m["mu"][:, : nsteps + 1]))


def test_the_exactness_bound_holds_for_every_family_of_check_b():
	"""Every partial sum of every step fits the mantissa, for every spelling (the duplicates' pieces enter with their own absolute values):
	at most 4 j + 7 bits at step j where every entry is an integer, 14 j + 16 with a long row of 2**-10 entries."""
	for name in cc.CHEB_NAMES:
		for dt in (F64, F32):
			nsteps, mant = cc.cheb_steps(name, dt), cc.MANT[np.dtype(dt)]
			worst = 0.0
			for sp in cc.SPELLINGS:
				R = cc.raw(name, sp)
				m = cc.exact_chebyshev(R, cc.rademacher(R.M.n, 17, 0), nsteps)
				assert m["K"] == nsteps and cc.proven_steps(m["bits"], mant) == nsteps, (name, sp, m["bits"])
				if sp == "canonical":
					slope, const = (14, 16) if name.startswith("longrow") else (4, 7)
					assert all(b <= slope * j + const for j, b in enumerate(m["bits"])), (name, sp, m["bits"])
				assert m["sum_bits"] < mant, (name, sp, m["sum_bits"])  # the sum of all w_k is exact as well
				assert m["mu_bits"][0] < mant and m["mu_bits"][1] < mant
				worst = max(worst, max(m["bits"]))
			print(f"[csr-edges] model {name} {np.dtype(dt).name}: {nsteps} steps, {worst:.1f} of {mant} bits")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["float64", "float32"])
def test_lanczos_inputs_are_insensitive_to_the_summation_order(oracle, dtype):
	"""alpha, beta of the oracle against oracle.np_lanczos whose product scatters the entries of the `dups` spelling in a random order: the
	deviation, relative to the tridiagonal's largest entry, stays within 1 / 100 of check (c)'s bar (1e-10 in fp64, 3e-4 in fp32) for every family
	and orth used there. fp32 leaves n < 12 out (deg = n: the last steps amplify any rounding)."""
	bar = (1e-10 if dtype == F64 else 3e-4) / 100.0
	worst = (0.0, None)
	for name in cc.LANCZOS_NAMES:
		M = cc.family(name, "spd")
		n = M.n
		if dtype == F32 and n < 12:
			continue
		A = M.scipy(dtype)
		matvec = cc.scatter_matvec(cc.raw(name, "dups", "spd"), dtype, seed=n)
		deg = min(12, n)
		V = cc.rademacher(n, 2, 77).astype(dtype)
		for orth in (0, 3, 5, 12):
			o = min(orth, deg)
			for c in range(V.shape[1]):
				al, be = np.zeros(deg + 1, dtype), np.zeros(deg + 1, dtype)
				st = oracle.lanczos(A, V[:, c].copy(), deg, 1e-8, o, al, be, np.zeros((n, max(o, 2)), dtype, order="F"))
				al2, be2 = np.zeros(deg + 1, dtype), np.zeros(deg + 1, dtype)
				st2 = oracle.np_lanczos(matvec, V[:, c].copy(), deg, 1e-8, o, al2, be2, np.zeros((n, max(o, 2)), dtype, order="F"))
				assert st == st2 == deg, (name, orth, st, st2)
				scale = float(np.max(np.abs(al[:deg])))
				e = max(float(np.max(np.abs(al[:deg].astype(F64) - al2[:deg]))), float(np.max(np.abs(be[:deg].astype(F64) - be2[:deg])))) / scale
				if e > worst[0]:
					worst = (e, (name, orth))
				assert e <= bar, f"{name} orth={orth}: {e:.3e} above {bar:g}"
	print(f"[csr-edges] insensitivity {np.dtype(dtype).name}: worst {worst[0]:.3e} ({worst[0] / bar:.3f} of the bar / 100) at {worst[1]}")


def test_row_order_of_every_spelling_is_a_permutation():
	"""The host analysis (slq_debug_csr_layout, no device) under SLQ_REORDER=2 on every family and spelling: the row order is a permutation of
	0 .. n-1. On a pattern that is not symmetric (nonsym) the Cuthill-McKee search from the far end of a component need not lead back to its
	starting row; the order then came out short of the chunk and the copy into the permutation read past it."""
	import _layout_cases as lc

	class Pattern:
		pass

	for name in cc.ALL_NAMES:
		for sp in cc.SPELLINGS:
			R = cc.raw(name, sp)
			A = Pattern()
			A.shape, A.nnz, A.indptr, A.indices = R.M.shape, R.nnz, R.rowptr.copy(), R.colind.copy()
			d = lc.decide(A, "reorder2_tiles0")
			assert d["reordered"] == int(R.nnz > 0) and not d["have_tiles"], (name, sp, d["reordered"])
			if R.nnz:
				assert np.array_equal(np.sort(d["perm"]), np.arange(R.M.n)), (name, sp)
