#!/usr/bin/env python3
"""Differential check of the host key generators against the REFERENCE, on randomised arguments under fixed seeds.

run(api) is one fixed sequence of generator calls.  make_golden.py f9 runs it on the reference's generators (build container only) and
stores every result in generator_cases.npz; tests/test_keygen_families.py::test_generators_against_reference_randomised runs it on
keynet_amd.keys / keynet_amd.sparse and must reproduce each stored result: identical dense values, identical stored CSR triplets
(the stored order feeds later products), the same dtype, and the same RNG consumption (the next np.random.rand() after the call
under the same seed)."""
import numpy as np
import scipy.sparse

FUNCTIONS = ('givens_orthogonal', 'diagonally_dominant_doubly_stochastic', 'hierarchical_block_permute', 'hierarchical_block_permutation_matrix',
             'diagonal_affine_to_linear', 'sparse_affine_to_linear', 'sparse_permutation_matrix', 'DiagonalTiledMatrix')


def run(api):
    """api: an object with the generators named in FUNCTIONS.  Returns {key: array}: the results of the whole case sequence."""
    rng = np.random.RandomState(123)
    out = {}

    def matrix(key, M):
        M = scipy.sparse.csr_matrix(M) if not scipy.sparse.issparse(M) else M.tocsr()
        (out[key + '.indptr'], out[key + '.indices'], out[key + '.data']) = (np.asarray(M.indptr), np.asarray(M.indices), np.asarray(M.data))
        out[key + '.shape'] = np.array(M.shape, dtype=np.int64)

    def seeded(key, seed, f):
        np.random.seed(seed)
        r = f()
        out[key + '.rng_next'] = np.array(np.random.rand())          # same number of draws -> same next value
        return r

    for t in range(12):
        (n, k) = (int(rng.randint(2, 40)), int(rng.randint(1, 60)))
        (R, Ri) = seeded('givens.%d' % t, t, lambda: api.givens_orthogonal(n, k, withinverse=True))
        matrix('givens.%d.M' % t, R); matrix('givens.%d.Minv' % t, Ri)
    for t in range(10):
        (n, k) = (int(rng.randint(6, 48)), int(rng.randint(2, 7)))
        (R, Ri) = seeded('stochastic.%d' % t, 100 + t, lambda: api.diagonally_dominant_doubly_stochastic(n, k, withinverse=True))
        matrix('stochastic.%d.M' % t, R); matrix('stochastic.%d.Minv' % t, Ri)
    for t in range(12):
        (H, C) = (int(rng.choice([16, 32, 64])), int(rng.randint(1, 4)))
        levels = [list(range(0, d + 1)) for d in range(0, int(np.log2(H)) - 3 + 1)][int(rng.randint(0, int(np.log2(H)) - 2))]
        twist = bool(rng.randint(0, 2))
        img = rng.rand(H, H, C).astype(np.float32)
        out['blockpermute.%d.image' % t] = seeded('blockpermute.%d' % t, 200 + t, lambda: api.hierarchical_block_permute(img, (2, 2), levels, min_blocksize=8, twist=twist))
        (R, Ri) = seeded('blockpermutation.%d' % t, 300 + t, lambda: api.hierarchical_block_permutation_matrix((H, H, C), (2, 2), levels, min_blocksize=8, twist=twist, withinverse=True))
        matrix('blockpermutation.%d.M' % t, R); matrix('blockpermutation.%d.Minv' % t, Ri)
    img = rng.rand(24, 40, 2)
    out['blockpermute.odd.image'] = seeded('blockpermute.odd', 7, lambda: api.hierarchical_block_permute(img, (3, 5), [0]))
    for t in range(10):
        n = int(rng.randint(1, 30))
        d = scipy.sparse.diags(rng.rand(n) + 0.5)
        bias = rng.randn(n, 1) * (rng.rand(n, 1) > 0.3) if t % 3 else None
        for fmt in ('dia', 'csr', 'coo'):
            A = d.asformat(fmt)
            (R, Ri) = api.diagonal_affine_to_linear(A, bias, withinverse=True)
            matrix('diagaffine.%d.%s.L' % (t, fmt), R); matrix('diagaffine.%d.%s.Linv' % (t, fmt), Ri)
            matrix('sparseaffine.%d.%s' % (t, fmt), api.sparse_affine_to_linear(A, bias))
    for t in range(6):
        n = int(rng.randint(1, 50))
        (R, Ri) = seeded('permutation.%d' % t, 400 + t, lambda: api.sparse_permutation_matrix(n, withinverse=True))
        matrix('permutation.%d.M' % t, R); matrix('permutation.%d.Minv' % t, Ri)
        (h, H) = (int(rng.randint(1, 6)), int(rng.randint(3, 20)))
        B = rng.rand(h, h).astype(np.float32)
        R = api.DiagonalTiledMatrix(B, shape=(H, H))
        out['diagtiled.%d.dense.blocks' % t] = np.array(list(R), dtype=np.int64).reshape(-1, 3)
        matrix('diagtiled.%d.dense' % t, R.tocsr())
        Bs = scipy.sparse.random(h, h, density=0.6, format='csr', dtype=np.float32, random_state=t)
        R = api.DiagonalTiledMatrix(Bs, shape=(H, H + 1))
        out['diagtiled.%d.sparse.blocks' % t] = np.array(list(R), dtype=np.int64).reshape(-1, 3)
        matrix('diagtiled.%d.sparse' % t, R.tocsr())
    return out


def mismatches(stored, own):
    """Keys whose arrays differ between a stored run and this one (values; dtypes too, except for CSR index arrays)."""
    bad = sorted(set(stored) ^ set(own))
    for k in sorted(set(stored) & set(own)):
        (a, b) = (np.asarray(stored[k]), np.asarray(own[k]))
        if not (a.shape == b.shape and np.array_equal(a, b) and (k.endswith(('.indptr', '.indices')) or a.dtype == b.dtype)):
            bad.append(k)
    return bad
