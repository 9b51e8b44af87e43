"""The keyed cell of the GPU modules: a parameter chain, a seeded oracle secret, a context, and Galois keys that the oracle
generates and the context loads at their first use.  A module subclasses KeyedCell for what is its own -- its chain, its
seeds, its inputs, its oracle results -- and keeps its fixture, which cell_cache fills; contexts stay module-scoped."""
import numpy as np

import inner_sum_model as model
from helpers import make_context, make_params, random_cts


class KeyedCell:
    def __init__(self, P, seed):
        self.P = P
        P.seed(seed)
        self.sk = P.keygen_secret()
        self.ctx = make_context(P)
        self.evks, self._cached = {}, {}

    def key(self, g):
        if g not in self.evks:
            self.evks[g] = self.P.keygen_galois(self.sk, g)
            self.ctx.load_galois_key(g, self.evks[g])
        return self.evks[g]

    __call__ = key  # the key source tests/inner_sum_model.py takes

    def keys(self, gl):
        return [self.key(g) for g in gl]

    def load_inner_sum(self, n):
        """the keys of InnerSum(n), a power of two, in the order of its rotations"""
        return self.keys(self.P.inner_sum_galois_elements(n))

    def load_for(self, batch, n):
        """the keys of InnerSum(., batch, n) for any n"""
        return self.keys(self.ctx.inner_sum_general_elements(batch, n))

    def at(self, nl):
        """the first nl limbs of the cell's ciphertexts `cts`"""
        return np.ascontiguousarray(self.cts[:, :, :nl])

    def cached(self, name, fn):
        """fn(), computed once per name and left unchanged: arrays (a tuple's too) are made read-only"""
        if name not in self._cached:
            w = fn()
            for a in w if isinstance(w, tuple) else (w,):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._cached[name] = w
        return self._cached[name]

    def close(self):
        self.ctx.close()


def cell_cache(make):
    """Body of a module-scoped fixture: yields get(*key), which builds make(*key) at first use, and closes every cell
    it made once the module is done -- the later ones too when a close() raises; the first such error is raised then"""
    made, errors = {}, []

    def get(*key):
        if key not in made:
            made[key] = make(*key)
        return made[key]

    yield get
    for c in made.values():
        try:
            c.close()
        except Exception as e:
            errors.append(e)
    if errors:
        raise errors[0]


class GeneralSumCell(KeyedCell):
    """One degree on the reference-style chain: L = 5, K = 2, three five-limb ciphertexts; the results of
    tests/inner_sum_model.py are computed once per (level, batch, n).  Shared by test_inner_sum_general.py and
    test_inner_sum_census.py, each with a cell of its own."""

    def __init__(self, oracle, log_n):
        P = make_params(oracle, log_n, 5)
        assert (P.L, P.K) == (5, 2)
        super().__init__(P, 7000 + log_n)
        self.cts = random_cts(P, 3, 5, seed=900 + log_n)
        self.cts.setflags(write=False)

    def want(self, nl, batch, n):
        def make():
            self.load_for(batch, n)
            return np.stack([model.inner_sum(self.P, c, batch, n, self) for c in self.at(nl)])
        return self.cached(("sum", nl, batch, n), make)

    def matrix(self, nl, rows):
        def make():
            self.load_for(1, rows)
            pt = self.P.encode(np.random.default_rng(rows + nl).integers(0, 2**63, size=rows, dtype=np.uint64), nl=nl)
            return pt, np.stack([model.matrix_inner_sum(self.P, c, pt, rows, self) for c in self.at(nl)])
        return self.cached(("matrix", nl, rows), make)
