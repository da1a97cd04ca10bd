"""CSR inputs the C-ABI admits and no other test feeds (tests/test_csr_cases_cpu.py, tests/test_gpu_csr_edges.py): small seeded
matrix families, five spellings of each as raw (rowptr, colind, vals) - rows unsorted, reversed, with duplicate columns, stored zeros
and cancelling pairs -, and exact models of the product and of the Chebyshev recurrence. No GPU, no oracle import at module level.

Every value is an integer numerator over 2**shift (Matrix.shift: 0 for the integer families, 6 for k/64, 10 where a long row of
+-2**-10 entries is present), so that a spelling's pieces sum exactly and a model can say in integers which device sums are exact:
a float sum whose terms are multiples of one quantum q, and whose absolute terms add up to less than 2**mant q, is exact in every order, with or without fma."""

import math

import numpy as np

F64, F32 = np.float64, np.float32
MANT = {np.dtype(F64): 53, np.dtype(F32): 24}
OFFSETS = (1, 2, 3, 7, 61)
SPELLINGS = ("canonical", "shuffled", "reversed", "dups", "zeros")
H = 16.0  # half-width of the Chebyshev bounds (-16, 16): a power of two, every scaling by 1 / h or 2 / h is exact


class Matrix:
	"""A matrix as canonical COO triplets (sorted by row, then column; every position once): value = num / 2**shift."""

	def __init__(self, name, shape, rows, cols, num, shift, symmetric):
		order = np.lexsort((cols, rows))
		self.name, self.shape, self.shift, self.symmetric = name, (int(shape[0]), int(shape[1])), int(shift), bool(symmetric)
		self.rows, self.cols, self.num = rows[order].astype(np.int64), cols[order].astype(np.int64), num[order].astype(np.int64)
		assert len(set(zip(self.rows.tolist(), self.cols.tolist()))) == len(self.rows), name
		for z in (self.rows, self.cols, self.num):
			z.setflags(write=False)

	@property
	def n(self):
		return self.shape[0]

	@property
	def nnz(self):
		return len(self.rows)

	def scipy(self, dtype):
		"""The canonical CSR (sorted, no duplicates) in `dtype`."""
		import scipy.sparse as sp

		A = sp.csr_matrix((self.num / 2.0**self.shift, (self.rows, self.cols)), shape=self.shape).astype(dtype)
		A.sort_indices()
		return A

	def abs_row_sums(self):
		s = np.zeros(self.shape[0], dtype=np.int64)
		np.add.at(s, self.rows, np.abs(self.num))
		return s / 2.0**self.shift


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def _upper_pairs(n, offsets, rng, keep):
	out = [np.zeros((0, 2), dtype=np.int64)]
	for o in offsets:
		if o < n:
			i = np.arange(n - o, dtype=np.int64)
			k = rng.random(n - o) < keep
			out.append(np.stack([i[k], i[k] + o], axis=1))
	return np.concatenate(out)


def _band_pattern(n, rng, offsets=OFFSETS):
	"""(upper pairs i < j, emptied mask): every offset's entries kept with probability 0.65, about 2 % of the indices emptied (n >= 63: one at least)."""
	up = _upper_pairs(n, offsets, rng, 0.65)
	emptied = rng.random(n) < 0.02
	if n >= 63 and not emptied.any():
		emptied[int(rng.integers(n))] = True
	up = up[~(emptied[up[:, 0]] | emptied[up[:, 1]])]
	return up, emptied


def _grid_pattern(m, rng):
	idx = np.arange(m * m, dtype=np.int64).reshape(m, m)
	e = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], axis=1), np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()], axis=1)])
	return e[rng.random(len(e)) < 0.75], np.zeros(m * m, dtype=bool)


def _symmetric(name, n, up, emptied, rng, values, long=None):
	"""The symmetric matrix of the upper pairs `up` and a diagonal on every index that is not emptied. values "integer": off-diagonals
	+-1, diagonal in -2 .. 2 (not 0); "spd": off-diagonals k / 64, 0 < |k| <= 64, diagonal = absolute row sum (a multiple of 1 / 64 as it is) + 1.
	long = (r, cols): row and column r replaced by entries of +-2**-10 at `cols`."""
	shift = 0 if values == "integer" else 6
	off = rng.choice([-1, 1], len(up)) if values == "integer" else rng.integers(1, 65, len(up)) * rng.choice([-1, 1], len(up))
	if long is not None:
		r, lc = long
		keep = (up[:, 0] != r) & (up[:, 1] != r)
		up, off = up[keep], off[keep] * 2 ** (10 - shift)
		pairs = np.stack([np.minimum(lc, r), np.maximum(lc, r)], axis=1)
		up, off = np.concatenate([up, pairs]), np.concatenate([off, rng.choice([-1, 1], len(lc))])
		emptied = emptied.copy()
		emptied[r] = False
		shift = 10
	rows, cols, num = np.concatenate([up[:, 0], up[:, 1]]), np.concatenate([up[:, 1], up[:, 0]]), np.concatenate([off, off])
	d = np.flatnonzero(~emptied)
	if values == "integer":
		dv = rng.choice([-2, -1, 1, 2], len(d)) * 2**shift
	else:
		s = np.zeros(n, dtype=np.int64)
		np.add.at(s, rows, np.abs(num))
		unit = 2 ** (shift - 6)  # numerators per 1 / 64
		dv = -(-s[d] // unit) * unit + 2**shift
	M = Matrix(name, (n, n), np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([num, dv]), shift, True)
	if values == "integer":
		assert M.abs_row_sums().max(initial=0) <= 16, name
	return M


def _name_seed(name):
	return [ord(c) for c in name]


def band(n, values="integer"):
	rng = np.random.default_rng([1, n] + _name_seed(values))
	up, emptied = _band_pattern(n, rng)
	return _symmetric(f"band{n}-{values}", n, up, emptied, rng, values)


def grid(m, values="integer"):
	rng = np.random.default_rng([2, m] + _name_seed(values))
	up, emptied = _grid_pattern(m, rng)
	return _symmetric(f"grid{m}-{values}", m * m, up, emptied, rng, values)


def longrow(n, r, L, values="integer"):
	"""`band` with row and column r replaced by L entries of +-2**-10 (they must stay that small: with entries of order 1 the outlier
	eigenvalue makes the Lanczos recurrence sensitive to the summation order)."""
	rng = np.random.default_rng([3, n, r, L] + _name_seed(values))
	up, emptied = _band_pattern(n, rng)
	lc = rng.permutation(np.delete(np.arange(n, dtype=np.int64), r))[:L]
	assert len(lc) == L
	return _symmetric(f"longrow{n}_{r}_{L}-{values}", n, up, emptied, rng, values, long=(r, lc))


def far(n=8200, values="integer"):
	"""`band` plus an offset of 4100: entries further than 4096 rows away, 0.65 of them per row."""
	rng = np.random.default_rng([4, n] + _name_seed(values))
	up, emptied = _band_pattern(n, rng, OFFSETS + (4100,))
	return _symmetric(f"far{n}-{values}", n, up, emptied, rng, values)


def far7(n=8200, values="integer"):
	"""Offsets 1, 2, 3 and 4100 .. 4106: 4.5 entries per row further than 4096 rows away - above the 4 per row from which a plan
	takes the stored-u sequence (the gathers are no longer served from cache) - and absolute row sums still <= 16."""
	rng = np.random.default_rng([5, n] + _name_seed(values))
	up, emptied = _band_pattern(n, rng, (1, 2, 3) + tuple(range(4100, 4107)))
	return _symmetric(f"far7_{n}-{values}", n, up, emptied, rng, values)


def nonsym(n):
	"""The strict upper part of `band`, scaled by 2."""
	B = band(n)
	k = B.cols > B.rows
	return Matrix(f"nonsym{n}", (n, n), B.rows[k], B.cols[k], 2 * B.num[k], 0, False)


def zero(n):
	e = np.zeros(0, dtype=np.int64)
	return Matrix(f"zero{n}", (n, n), e, e, e, 0, True)


def rect(m, n):
	"""A rectangular m x n matrix of about four integer entries per row, |value| <= 3 (the Gram operator's B)."""
	rng = np.random.default_rng([6, m, n])
	rows = np.repeat(np.arange(m, dtype=np.int64), 4)
	cols = rng.integers(0, n, len(rows))
	key = np.unique(rows * n + cols)
	rows, cols = key // n, key % n
	num = rng.integers(1, 4, len(rows)) * rng.choice([-1, 1], len(rows))
	return Matrix(f"rect{m}x{n}", (m, n), rows, cols, num, 0, False)


BAND_NS = (1, 2, 5, 63, 64, 65, 257, 1000)
LONGROWS = ((1000, 999, 65), (1000, 0, 999), (4096, 17, 130), (4096, 4000, 300))
_FAMILIES = {}


def family(name, values="integer"):
	"""A family member by name, built once: band<n>, grid<m>, longrow<n>_<r>_<L>, far, far7, nonsym<n>, zero<n>."""
	key = (name, values)
	if key not in _FAMILIES:
		if name.startswith("band"):
			M = band(int(name[4:]), values)
		elif name.startswith("grid"):
			M = grid(int(name[4:]), values)
		elif name.startswith("longrow"):
			M = longrow(*(int(x) for x in name[7:].split("_")), values=values)
		elif name == "far":
			M = far(values=values)
		elif name == "far7":
			M = far7(values=values)
		elif name.startswith("nonsym"):
			M = nonsym(int(name[6:]))
		elif name.startswith("zero"):
			M = zero(int(name[4:]))
		else:
			raise KeyError(name)
		_FAMILIES[key] = M
	return _FAMILIES[key]


CHEB_NAMES = ("band1000", "grid64", "grid70", "far", "far7", "longrow4096_17_130")  # check (b)
LANCZOS_NAMES = ("band5", "band65", "band1000", "longrow1000_0_999", "grid64", "grid70", "longrow4096_17_130", "longrow4096_4000_300", "far", "far7")  # check (c)


def cheb_steps(name, dtype):
	"""Steps of check (b): 10 in fp64 and 4 in fp32, where the partial sums need 4 j + 7 bits at step j. A long row's entries of 2**-10 refine
	the quantum by 10 more bits per step (row r reads what it wrote two steps earlier): 14 j + 15 bits, which proves 3 steps in fp64 and 1 in fp32."""
	f64 = np.dtype(dtype) == np.dtype(F64)
	if name.startswith("longrow"):
		return 3 if f64 else 1
	return 10 if f64 else 4


ALL_NAMES = (tuple(f"band{n}" for n in BAND_NS) + ("grid64", "grid70") + tuple("longrow%d_%d_%d" % t for t in LONGROWS)
             + ("far", "far7") + tuple(f"nonsym{n}" for n in (5, 65, 1000)) + ("zero65", "zero5000"))  # fmt: skip


# ---- spellings --------------------------------------------------------------------------------------------------------------
class Raw:
	"""One spelling: rowptr, colind (int32) and the numerators (int64) of its stored entries, in storage order."""

	def __init__(self, M, spelling, rows, cols, num):
		self.M, self.spelling = M, spelling
		self.rows, self.colind, self.num = rows.astype(np.int64), cols.astype(np.int32), num.astype(np.int64)
		assert np.all(np.diff(self.rows) >= 0)
		self.rowptr = np.zeros(M.shape[0] + 1, dtype=np.int32)
		np.cumsum(np.bincount(self.rows, minlength=M.shape[0]), out=self.rowptr[1:])
		for z in (self.rows, self.colind, self.num, self.rowptr):
			z.setflags(write=False)

	@property
	def nnz(self):
		return len(self.colind)

	def vals(self, dtype):
		v = (self.num / 2.0**self.M.shift).astype(dtype)
		assert np.array_equal(v.astype(np.float64) * 2.0**self.M.shift, self.num)  # representable
		return v

	def dense_num(self):
		"""The numerators summed into a dense int64 matrix (small matrices: the CPU test's comparison of the spellings)."""
		D = np.zeros(self.M.shape, dtype=np.int64)
		np.add.at(D, (self.rows, self.colind.astype(np.int64)), self.num)
		return D


def _outside(M, rng, count):
	"""Up to `count` distinct positions outside M's pattern, near the diagonal (4 .. 40 columns to the right, wrapped)."""
	nr, nc = M.shape
	have = set((M.rows * nc + M.cols).tolist())
	out = []
	for _ in range(20 * count):
		if len(out) == count:
			break
		i = int(rng.integers(nr))
		j = (i + int(rng.integers(4, 41))) % nc
		if i * nc + j not in have:
			have.add(i * nc + j)
			out.append((i, j))
	return out


def spell(M, spelling):
	"""The same mathematical matrix as raw CSR arrays:
	canonical  rows sorted, every position once;
	shuffled   the columns of every row in random order;
	reversed   descending columns;
	dups       a third of the entries split into two or three pieces whose sum is exact - adjacent in the (sorted) even rows, apart in the (shuffled) odd rows;
	zeros      sorted rows with stored zeros (one of them in an otherwise empty row where there is one) and +v / -v pairs at positions outside the pattern."""
	rng = np.random.default_rng([7, SPELLINGS.index(spelling)] + _name_seed(M.name))
	rows, cols, num = M.rows, M.cols, M.num
	if spelling == "canonical":
		return Raw(M, spelling, rows, cols, num)
	if spelling == "shuffled":
		order = np.lexsort((rng.random(len(rows)), rows))
		return Raw(M, spelling, rows[order], cols[order], num[order])
	if spelling == "reversed":
		order = np.lexsort((-cols, rows))
		return Raw(M, spelling, rows[order], cols[order], num[order])
	if spelling == "dups":
		r2, c2, v2, pos = [], [], [], []
		pick = rng.random(len(rows)) < 1.0 / 3.0
		if len(rows) and not pick.any():
			pick[0] = True
		for k in range(len(rows)):
			v = int(num[k])
			pieces = [v]
			if pick[k]:
				a = int(rng.integers(-2 * abs(v) - 1, 2 * abs(v) + 2))
				a = 2 * v if a in (0, v) else a
				pieces = [a, v - a]
				if rng.random() < 0.5:
					b = int(rng.integers(1, abs(v) + 2))
					pieces = [a, b, v - a - b]
			odd = int(rows[k]) % 2 == 1
			for q, p in enumerate(pieces):
				r2.append(rows[k]), c2.append(cols[k]), v2.append(p)
				pos.append(rng.random() if odd else k + q / 4.0)  # odd rows: anywhere in the row; even rows: behind one another
		r2, c2, v2, pos = np.array(r2, dtype=np.int64), np.array(c2, dtype=np.int64), np.array(v2, dtype=np.int64), np.array(pos)
		order = np.lexsort((pos, r2))
		return Raw(M, spelling, r2[order], c2[order], v2[order])
	if spelling == "zeros":
		extra = _outside(M, rng, max(2, M.nnz // 8))
		nz = len(extra) // 2
		r2, c2, v2 = list(rows), list(cols), list(num)
		empty = np.flatnonzero(np.bincount(rows, minlength=M.shape[0]) == 0)
		if len(empty):
			i = int(empty[0])
			r2.append(i), c2.append((i + 1) % M.shape[1]), v2.append(0)
		for i, j in extra[:nz]:
			r2.append(i), c2.append(j), v2.append(0)
		for i, j in extra[nz:]:
			v = int(rng.integers(1, 4)) * 2**M.shift
			r2 += [i, i]
			c2 += [j, j]
			v2 += [v, -v]
		r2, c2, v2 = np.array(r2, dtype=np.int64), np.array(c2, dtype=np.int64), np.array(v2, dtype=np.int64)
		order = np.lexsort((np.arange(len(r2)), c2, r2))
		return Raw(M, spelling, r2[order], c2[order], v2[order])
	raise KeyError(spelling)


def stored_exactly_symmetric(R, rows_sorted_by_builder=False):
	"""Whether the CSR as stored qualifies for the upper-triangle copy: every row strictly ascending (sorted, no duplicate column) and every
	stored off-diagonal entry mirrored by a stored entry of equal value. rows_sorted_by_builder: the builder permutes the rows and sorts each on the
	way (equal columns keep the caller's order), so only duplicates and unmirrored entries count."""
	rows, cols, num = R.rows, R.colind.astype(np.int64), R.num
	if rows_sorted_by_builder:
		order = np.lexsort((cols, rows))  # (stable)
		rows, cols, num = rows[order], cols[order], num[order]
	if np.any(np.diff(cols)[rows[1:] == rows[:-1]] <= 0):
		return False
	n = R.M.shape[1]
	key = rows * n + cols  # ascending now
	at = np.searchsorted(key, cols * n + rows)
	at = np.minimum(at, max(len(key) - 1, 0))
	return bool(len(key) == 0 or (np.all(key[at] == cols * n + rows) and np.all(num[at] == num)))


_RAW = {}


def raw(name, spelling, values="integer"):
	key = (name, spelling, values)
	if key not in _RAW:
		_RAW[key] = spell(family(name, values), spelling)
	return _RAW[key]


# ---- exact models -----------------------------------------------------------------------------------------------------------
def exact_product(R, X):
	"""(Y, bits): A X for integer X in int64 from the COO triplets of the spelling `R` as stored (np.add.at, no canonicalisation), returned as
	the exact float64 array Y = numerators / 2**shift; bits = log2 of the largest sum of absolute terms in units of the quantum 2**-shift:
	below the mantissa, every partial sum of the device's product is an exact float in any order."""
	X = np.asarray(X)
	assert X.dtype.kind == "i"
	X = X.astype(np.int64).reshape(R.M.shape[1], -1)
	Y = np.zeros((R.M.shape[0], X.shape[1]), dtype=np.int64)
	ci = R.colind.astype(np.int64)
	for c0 in range(0, X.shape[1], 16):
		np.add.at(Y[:, c0 : c0 + 16], R.rows, R.num[:, None] * X[:, c0 : c0 + 16][ci])
	B = np.zeros(R.M.shape[0], dtype=np.int64)  # (the bound: a row's absolute entries times the largest |x|)
	np.add.at(B, R.rows, np.abs(R.num))
	bits = math.log2(max(int(B.max(initial=0)) * int(np.abs(X).max(initial=0)), 1))
	assert bits < 53
	return Y / 2.0**R.M.shift, bits


def _int_csr(R, absolute=False):
	import scipy.sparse as sp

	num = np.abs(R.num) if absolute else R.num
	return sp.csr_matrix((num, (R.rows, R.colind.astype(np.int64))), shape=R.M.shape, dtype=np.int64)  # (duplicates summed in int64: exact)


def exact_chebyshev(R, V, nsteps, h=H):
	"""The scaled integer recurrence of w_0 = V, w_1 = A w_0 / h, w_{j+1} = 2 A w_j / h - w_{j-1} (bounds (-h, h), h a power of two) on the
	spelling R: Z_j = (h 2**shift)**j w_j are integers, Z_1 = N Z_0, Z_{j+1} = 2 N Z_j - (h 2**shift)**2 Z_{j-1} with N the numerators.

	Returns dict(w, bits, mu, mu_bits, sum_bits):
	 w[k]       w_k as an exact float64 array, k = 0 .. K, K <= nsteps the last step whose Z fits int64 (the recurrence stops where bits reaches 62);
	 bits[j]    log2 of the largest sum of absolute terms of step j (the one that writes w_{j+1}) in units of ITS quantum (h 2**shift)**-(j+1):
	            max_i (2 sum_k |N_ik| |Z_j[k]| + (h 2**shift)**2 |Z_{j-1}[i]|). Where bits[j] < mant, every partial sum of the row's product, its
	            scaling by 1 / h or 2 / h and the subtraction of w_{j-1} are exact in that format, in any order, fused or not;
	 mu[:, k]   the moments v . T_k(A / h) v as the device forms them (mu_0 = |v|^2, mu_1 = w_1 . w_0, mu_{2j+1} = 2 w_{j+1} . w_j - mu_1,
	            mu_{2j+2} = 2 |w_{j+1}|^2 - mu_0), exact floats, NaN where not computed;
	 mu_bits[k] log2 of 2 sum_i |w_a[i]| |w_b[i]| + |mu_0 or mu_1| in units of the products' quantum: below mant, moment k is exact;
	 sum_bits   log2 of max_i sum_k |w_k[i]| in units of the finest quantum (h 2**shift)**-K: below mant, sum_k w_k is exact in any order."""
	V = np.asarray(V)
	assert V.dtype.kind == "i" and float(h) == 2.0 ** round(math.log2(h))
	N, NA = _int_csr(R), _int_csr(R, absolute=True).astype(np.float64)
	s = int(round(math.log2(h))) + R.M.shift  # log2 of h 2**shift
	Z = [V.astype(np.int64).reshape(R.M.shape[0], -1)]
	bits = []
	for j in range(nsteps):
		bound = NA @ np.abs(Z[j]).astype(np.float64)  # (a float evaluation of an integer bound: relative error 1e-15)
		if j > 0:
			bound = 2.0 * bound + 2.0 ** (2 * s) * np.abs(Z[j - 1]).astype(np.float64)
		bits.append(math.log2(max(float(bound.max(initial=0.0)), 1.0)) + 1e-9)
		if bits[-1] >= 62:
			break
		Z.append(N @ Z[j] if j == 0 else 2 * (N @ Z[j]) - (Z[j - 1] << (2 * s)))
	K = len(Z) - 1
	w = [np.ldexp(Z[k].astype(np.float64), -s * k) for k in range(K + 1)]
	for k in range(K + 1):
		assert np.array_equal(np.ldexp(w[k], s * k).astype(np.int64), Z[k])  # (|Z_k| <= 2**bits[k-1] < 2**53: exact)
	P = Z[0].shape[1]
	mu, mu_bits = np.full((P, 2 * nsteps + 1), np.nan), np.full(2 * nsteps + 1, np.inf)

	def dot(a, b):
		"""(exact integers sum_i Z_a Z_b per column as Python ints, log2 of the largest sum of absolute products)"""
		ab = float((np.abs(Z[a]).astype(np.float64) * np.abs(Z[b]).astype(np.float64)).sum(axis=0).max(initial=0.0))
		if ab >= 2.0**62:
			return None, math.inf
		return [int(x) for x in (Z[a] * Z[b]).sum(axis=0)], math.log2(max(ab, 1.0))

	m0, _ = dot(0, 0)
	mu[:, 0], mu_bits[0] = m0, math.log2(max(max(m0), 1))
	m1 = None
	for k in range(1, 2 * K + 1):
		a, b = (k + 1) // 2, k // 2  # mu_k from w_a . w_b, a + b = k
		d, db = dot(a, b)
		if d is None:
			continue
		if k == 1:
			m1 = d
			mu[:, 1] = [math.ldexp(x, -s) for x in d]
			mu_bits[1] = db
			continue
		base = m0 if k % 2 == 0 else m1
		num = [2 * x - y * (1 << (s * (k - (k % 2)))) for x, y in zip(d, base)]  # mu_0 has quantum 1, mu_1 (h 2**shift)**-1: both in units of (..)**-k
		mu_bits[k] = math.log2(max(2.0 * 2.0**db + max(abs(y) for y in base) * 2.0 ** (s * (k - (k % 2))), 1.0))
		if mu_bits[k] < 53:
			mu[:, k] = [math.ldexp(x, -s * k) for x in num]
	tot = np.zeros(Z[0].shape, dtype=np.float64)
	for k in range(K + 1):
		tot += np.ldexp(np.abs(Z[k]).astype(np.float64), s * (K - k))
	return dict(w=w, bits=bits, mu=mu, mu_bits=mu_bits, sum_bits=math.log2(max(float(tot.max(initial=0.0)), 1.0)), K=K)


def proven_steps(bits, mant):
	"""How many leading steps of exact_chebyshev's `bits` stay below the mantissa."""
	k = 0
	while k < len(bits) and bits[k] < mant:
		k += 1
	return k


def rademacher(n, P, seed):
	return (np.random.default_rng([11, n, seed]).integers(0, 2, (n, P)) * 2 - 1).astype(np.int64)


def int_panel(n, P, seed, lim=7):
	return np.random.default_rng([12, n, seed]).integers(-lim, lim + 1, (n, P)).astype(np.int64)


def scatter_matvec(R, dtype, seed):
	"""x -> A x in `dtype` as a scatter over the stored entries of R in a random order: another summation order than any row loop."""
	order = np.random.default_rng([13, seed]).permutation(R.nnz)
	rows, cols, v = R.rows[order], R.colind.astype(np.int64)[order], R.vals(dtype)[order]

	def matvec(x):
		y = np.zeros(R.M.shape[0], dtype=dtype)
		np.add.at(y, rows, v * x[cols].astype(dtype))
		return y

	return matvec
